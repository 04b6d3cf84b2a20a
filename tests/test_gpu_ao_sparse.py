"""Sparse AO visibility on the GPU, bit for bit (include/trx.h: trx_trace_ao_visibility_sparse_dev, trx_ao_upsample_dev,
trx_render_image_sparse).  The sparse counts against trx_trace_ao_visibility_dev's own bytes at the represented pixels and
against the twin (tests/ao_visibility_twin.py subsampled, tests/ao_sparse_twin.py); the upsample against the numpy twin
fed the device's own records, and against trx_ao_filter_dev at stride 1; the host form against its composition; refusals,
the scratch's accounting and the ordering with a refit.  No cell and no pixel is left out of any comparison."""
import ctypes as C
import os

import numpy as np
import pytest

from ao_sparse_twin import ACCEPTED, EMPTY, FALLBACK, NO_SURFACE, ao_upsample, cell_pixels, class_counts, lo_size, sparse_counts
from helpers import ALL_SEMS, random_rays
from image_twin import TERM_DTYPE, ao_filter, shade_term, surface
from test_gpu_ao_visibility import UNIT, Case, make_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
FILL = 0x5A
N, EPS, SEM = 4, 0.01, 3
RADIUS = {"soup_52x44": 0.8, "cornell_tlas_48": 1.4}
STRIDES_PHASES = ((1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 8), (4, 0), (4, 15))


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"


def _torch():
    import torch
    return torch


def _buf(nbytes, fill=FILL):
    torch = _torch()
    return torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda")


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.fixture(scope="module")
def cases(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            base = name[:-len("_pipe")] if name.endswith("_pipe") else name
            plain = make_case(trx, orc, made, base)
            plain.radius = RADIUS.get(base, plain.radius)
            make_case(trx, orc, made, name)          # (a padded twin takes its base case's radius, as it stands now)
        return make_case(trx, orc, made, name)      # (which asks the library again which walk a twin takes)
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


def _on_the_unpadded_scene_too(case, run):
    """run(scene) on the case's scene; on a padded twin (the pipelined walk) also on the unpadded scene (the plain walk), which
    must give the same bytes."""
    got = run(case.sc)
    if case.base is not None:
        plain = run(case.base.sc)
        assert (got == plain).all(), "%s: %d bytes differ from the unpadded scene's" % (case.name, (got != plain).sum())
    return got


def _dense(case, d_prim, d_inst, n, radius, sem, frame0):
    torch = _torch()

    def run(sc):
        d_out = _buf(case.w * case.h)
        sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_out.data_ptr(), n, radius, sem=sem, frame0=frame0,
                                   ao_eps=EPS, d_primary_inst=d_inst.data_ptr())
        torch.cuda.synchronize()
        return d_out.cpu().numpy()
    return _on_the_unpadded_scene_too(case, run)


def _sparse(case, d_prim, d_inst, stride, phase, n, radius, sem, frame0, stream=0):
    """The low grid's bytes, after checking that the 64 bytes past them kept their fill."""
    torch = _torch()
    wlo, hlo = lo_size(case.w, case.h, stride)

    def run(sc):
        d_out = _buf(wlo * hlo + 64)
        sc.trace_ao_visibility_sparse_dev(case.view, case.w, case.h, stride, phase, d_prim.data_ptr(), d_out.data_ptr(), n, radius,
                                          sem=sem, frame0=frame0, ao_eps=EPS, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0,
                                          stream=stream)
        torch.cuda.synchronize()
        sc.check()
        raw = d_out.cpu().numpy()
        assert (raw[wlo * hlo:] == FILL).all(), "bytes past Wlo * Hlo were written"
        return raw[:wlo * hlo]
    return _on_the_unpadded_scene_too(case, run)


# ---- 1. the sparse counts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48", "instanced", "soup_52x44_pipe"])
def test_sparse_counts_are_the_dense_passs_bytes_and_the_twins(trx, orc, cases, name):
    """Strides 1..4 (every phase of 2, the first and last of 3 and 4), 1 / 8 / 64 samples, a finite radius and +inf under
    TRX_SEM_HLSL and TRX_SEM_CPU (64 samples under TRX_SEM_CPU); stride 2 under all eight semantics words; a non-null stream."""
    torch = _torch()
    case = cases(name)
    w, h = case.w, case.h
    st = torch.cuda.Stream()
    for sem in ALL_SEMS:
        d_prim, d_inst, prim, inst = case.primary(sem)
        if sem in (0, 3):
            configs = [(n, r) for n in ((1, 8, 64) if sem == 3 else (1, 8)) for r in (case.radius, INF) if n != 64 or r != INF]
            grids = STRIDES_PHASES
        else:
            configs, grids = [(4, case.radius)], ((2, sem % 4),)
        twin = {}
        for radius in sorted({r for _, r in configs}):
            twin[radius] = case.unoccluded(sem, prim, inst, 3, max(n for n, r in configs if r == radius), radius)
        for n, radius in configs:
            unocc, surf = twin[radius]
            want_twin = np.where(surf, unocc[:n].sum(0), NO_SURFACE).astype(np.uint8)
            dense = _dense(case, d_prim, d_inst, n, radius, sem, 3)
            assert (dense == want_twin).all(), "the dense pass left its twin"
            for k, (stride, phase) in enumerate(grids):
                got = _sparse(case, d_prim, d_inst, stride, phase, n, radius, sem, 3, stream=st.cuda_stream if k % 2 else 0)
                what = "%s sem %d n %d radius %g stride %d phase %d" % (name, sem, n, radius, stride, phase)
                want = sparse_counts(dense, w, h, stride, phase)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, "%s: %d of %d cells differ from the dense pass, first %s: %s != %s" % (
                    what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])
                assert (got == sparse_counts(want_twin, w, h, stride, phase)).all(), what + ": differs from the twin"
                if stride == 1:
                    assert (got == dense).all(), what
                if name == "soup_52x44" and (stride, phase) == (3, 8):
                    outside = ~cell_pixels(w, h, stride, phase)[2].reshape(-1)     # 52 and 44 are no multiples of 3
                    assert outside.sum() > 10 and (got[outside] == NO_SURFACE).all(), what
            surf_counts = dense[dense != NO_SURFACE]
            if n == 8 and radius != INF and sem in (0, 3):
                assert ((surf_counts > 0) & (surf_counts < 8)).any() and (dense == NO_SURFACE).any(), name + ": a vacuous frame"


def test_chunk_loops_give_the_same_cells(trx, orc, cases):
    """A scratch cap below the pass's need: samples in several chunks, tiles in several chunks, both; restored afterwards."""
    lib = trx.load()
    try:
        # (the transformed two-level scene, and the padded twin of the soup golden: chunks of the pipelined any-hit walk)
        for name, grids in (("instanced", ((2, 3), (3, 0))), ("soup_52x44_pipe", ((2, 3), (4, 5)))):
            case = cases(name)
            d_prim, d_inst, _, _ = case.primary(SEM)
            for stride, phase in grids:
                wlo, hlo = lo_size(case.w, case.h, stride)
                tiles = ((wlo + 7) // 8) * ((hlo + 7) // 8)
                assert tiles >= (6 if name == "instanced" else 4)
                lib.trx_debug_ao_scratch_cap(0)
                want = _sparse(case, d_prim, d_inst, stride, phase, 8, case.radius, SEM, 0)
                assert ((want > 0) & (want < 8)).any()
                for cap in (UNIT * tiles * 3, UNIT * tiles, UNIT * 4, UNIT * (tiles // 2 + 1) * 2, 1):
                    lib.trx_debug_ao_scratch_cap(cap)
                    got = _sparse(case, d_prim, d_inst, stride, phase, 8, case.radius, SEM, 0)
                    assert (got == want).all(), "%s stride %d cap %d: %d cells differ" % (name, stride, cap, (got != want).sum())
    finally:
        lib.trx_debug_ao_scratch_cap(0)


def test_sparse_refusals_leave_the_output_untouched(trx, cases):
    torch = _torch()
    case = cases("instanced")
    d_prim, d_inst, _, _ = case.primary(0)
    d_out = _buf(case.w * case.h)

    def call(stride=2, phase=0, n=4, radius=1.0, sem=0, inst=True, w=case.w):
        case.sc.trace_ao_visibility_sparse_dev(case.view, w, case.h, stride, phase, d_prim.data_ptr(), d_out.data_ptr(), n, radius, sem=sem,
                                               d_primary_inst=d_inst.data_ptr() if inst else 0)

    with pytest.raises(trx.TrxError, match="instance transforms") as e:
        call(inst=False)
    assert e.value.code == -1
    for kw, msg in (({"stride": 0}, "stride"), ({"stride": 5}, "stride"), ({"stride": 2, "phase": 4}, "phase"), ({"stride": 1, "phase": 1}, "phase"),
                    ({"stride": 4, "phase": 16}, "phase"), ({"n": 0}, "n_samples"), ({"n": 65}, "n_samples"), ({"radius": 0.0}, "ao_radius"),
                    ({"radius": float("nan")}, "ao_radius"), ({"sem": 8}, "semantics"), ({"w": 0}, "image")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            call(**kw)
        assert e.value.code == -1, kw
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    call()   # and the scene is still usable
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() != FILL).any()
    case.sc.check()


def test_device_bytes_count_the_scratch_once(trx, orc):
    torch = _torch()
    case = Case(trx, orc, "cornell_64")
    try:
        d_prim, d_inst, _, _ = case.primary(0)
        n, stride = 4, 2
        wlo, hlo = lo_size(case.w, case.h, stride)
        tiles = ((wlo + 7) // 8) * ((hlo + 7) // 8)
        # the rays launch of this size first, on the same stream: the launch slot's stack spill area is then sized for it
        d_rays = torch.zeros((tiles * n * 64 * 32,), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((tiles * n * 64,), dtype=torch.uint8, device="cuda")
        case.sc.trace_occluded_dev(d_rays.data_ptr(), tiles * n * 64, d_flags.data_ptr())
        torch.cuda.synchronize()
        before = case.sc.device_bytes
        _sparse(case, d_prim, d_inst, stride, 0, n, 1.4, 0, 0)
        first = case.sc.device_bytes
        assert first - before == tiles * n * UNIT
        _sparse(case, d_prim, d_inst, stride, 3, n, INF, 3, 0)
        _sparse(case, d_prim, d_inst, 4, 15, n, 1.4, 0, 0)
        _sparse(case, d_prim, d_inst, 3, 0, 1, 1.4, 0, 0)
        assert case.sc.device_bytes == first
    finally:
        case.close()


# ---- 2. the upsample ------------------------------------------------------------------------------------------------

class Frame:
    """The whole-image records of one frame as the library's passes leave them on the device, and on the host."""

    def __init__(self, trx, sc, view, w, h, radius, stream=0, dense=True):
        from tray_racing_amd import _lib as L
        self.w, self.h, self.n, self.view, self.radius = w, h, w * h, view, radius
        n = self.n
        self.d_prim, self.d_inst, self.d_attr, self.d_cnt = _buf(n * 8), _buf(n * 4), _buf(n * 24), _buf(n)
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), SEM, C.c_void_p(self.d_prim.data_ptr()),
                                                   C.c_void_p(self.d_inst.data_ptr()), C.c_void_p(stream)))
        sc.hit_attributes_primary_dev(view, w, h, self.d_prim.data_ptr(), self.d_attr.data_ptr(), d_inst=self.d_inst.data_ptr(), stream=stream)
        if dense:
            sc.trace_ao_visibility_dev(view, w, h, self.d_prim.data_ptr(), self.d_cnt.data_ptr(), N, radius, sem=SEM, frame0=0, ao_eps=EPS,
                                       d_primary_inst=self.d_inst.data_ptr(), stream=stream)

    def host(self, trx):
        _torch().cuda.synchronize()
        self.prim = self.d_prim.cpu().numpy().view(trx.HIT_DTYPE)
        self.attr = self.d_attr.cpu().numpy().view(trx.HIT_ATTR_DTYPE)
        self.cnt = self.d_cnt.cpu().numpy()
        return self

    def sparse(self, sc, stride, phase, stream=0):
        """The device's low grid for (stride, phase): a tensor of Wlo * Hlo bytes."""
        wlo, hlo = lo_size(self.w, self.h, stride)
        d_lo = _buf(wlo * hlo)
        sc.trace_ao_visibility_sparse_dev(self.view, self.w, self.h, stride, phase, self.d_prim.data_ptr(), d_lo.data_ptr(), N, self.radius,
                                          sem=SEM, frame0=0, ao_eps=EPS, d_primary_inst=self.d_inst.data_ptr(), stream=stream)
        return d_lo


class Synthetic:
    """Hand-made whole-image records on the device: depth steps, misses of both kinds, three normals, counts 0..N."""

    def __init__(self, trx, w, h, seed, misses=False):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.n = w, h, w * h
        self.prim = np.zeros(self.n, dtype=trx.HIT_DTYPE)
        self.prim["t"] = rng.choice(np.array([1.0, 1.01, 1.5, INF, 3.4028234663852886e38], dtype=np.float32), self.n, p=[.4, .3, .15, .1, .05])
        self.prim["prim"] = np.where(rng.random(self.n) < 0.08, 0xFFFFFFFF, rng.integers(0, 1000, self.n)).astype(np.uint32)
        if misses:
            self.prim["t"], self.prim["prim"] = INF, 0xFFFFFFFF
        self.attr = np.zeros(self.n, dtype=trx.HIT_ATTR_DTYPE)
        self.attr["normal"] = np.array([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]], dtype=np.float32)[rng.integers(0, 3, self.n)]
        self.cnt = np.where(surface(self.prim), rng.integers(0, N + 1, self.n), NO_SURFACE).astype(np.uint8)
        self.d_prim, self.d_attr = _dev(self.prim), _dev(self.attr)


def _golden_scene(trx, name):
    from tray_racing_amd import _lib
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = g["tri_verts"].shape[0]
    flat = trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n), [0, n])
    view = _lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    return flat, view, int(g["width"]), int(g["height"])


@pytest.fixture(scope="module")
def frames(trx):
    """name -> (scene, view, w, h, the frame with its host copies): traced once, read by every test."""
    made = {}

    def get(name):
        if name not in made:
            flat, view, w, h = _golden_scene(trx, name)
            sc = trx.Scene(flat)
            made[name] = (sc, view, w, h, Frame(trx, sc, view, w, h, RADIUS[name]).host(trx))
            sc.check()
        return made[name]
    yield get
    for sc, *_ in made.values():
        sc.close()


def _upsample(sc, fr, d_lo, stride, phase, r, tol, cos, attr, stream=0):
    d_term = _buf(fr.n * 4 + 64)
    sc.ao_upsample_dev(fr.w, fr.h, stride, phase, fr.d_prim.data_ptr(), d_lo.data_ptr(), d_term.data_ptr(), N, r, depth_tol=tol,
                       normal_cos=cos, d_attr=fr.d_attr.data_ptr() if attr else 0, stream=stream)
    return d_term


def _check_upsample(sc, fr, d_lo, lo, stride, phase, r, tol, cos, attr, what):
    d_term = _upsample(sc, fr, d_lo, stride, phase, r, tol, cos, attr)
    _torch().cuda.synchronize()
    raw = d_term.cpu().numpy()
    assert (raw[fr.n * 4:] == FILL).all(), what + ": bytes past width * height * 4 were written"
    got = raw[:fr.n * 4].view(TERM_DTYPE)
    want, cls = ao_upsample(fr.prim, fr.attr["normal"] if attr else None, lo, fr.w, fr.h, stride, phase, N, r, tol, cos, classes=True)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s stride %d phase %d r %d tol %g cos %g attr %d: %d pixels differ (first %s: %s vs %s)" % (
        what, stride, phase, r, tol, cos, attr, bad.size, divmod(int(bad[0]), fr.w)[::-1], got[bad[0]], want[bad[0]])
    return got, cls


@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_upsample_against_twin_on_the_goldens(trx, frames, name):
    sc, view, w, h, fr = frames(name)
    s = surface(fr.prim)
    assert 0.2 * s.size < s.sum() and (fr.cnt[s] <= N).all() and (fr.cnt[~s] == NO_SURFACE).all()
    for stride, phase in STRIDES_PHASES:
        d_lo = fr.sparse(sc, stride, phase)
        _torch().cuda.synchronize()
        lo = d_lo.cpu().numpy()
        assert (lo == sparse_counts(fr.cnt, w, h, stride, phase)).all()
        full = stride == 2 or phase == 0     # (every class at every phase of stride 2 and at one phase of the others)
        for r in (0, 1, 2):
            for attr in (True, False):
                for tol in ((0.0, 0.02, INF) if full else (0.02,)):
                    for cos in ((-1.0, 0.9, 1.0) if attr and full else (0.9,)):
                        got, cls = _check_upsample(sc, fr, d_lo, lo, stride, phase, r, tol, cos, attr, name)
                        assert not got.view(np.uint32)[~s].any()
                        if stride == 1:
                            d_flt = _buf(fr.n * 4)
                            sc.ao_filter_dev(w, h, fr.d_prim.data_ptr(), fr.d_cnt.data_ptr(), d_flt.data_ptr(), N, r, depth_tol=tol,
                                             normal_cos=cos, d_attr=fr.d_attr.data_ptr() if attr else 0)
                            _torch().cuda.synchronize()
                            assert (d_flt.cpu().numpy().view(np.uint32) == got.view(np.uint32)).all(), "stride 1 is not the filter"
                            assert (got.view(np.uint32) == ao_filter(fr.prim, fr.attr["normal"] if attr else None, fr.cnt, w, h, N, r, tol,
                                                                     cos).view(np.uint32)).all()
        if stride == 2 and phase == 0:
            # the three branches do something on these frames, on the device's own records too
            _, cls = _check_upsample(sc, fr, d_lo, lo, 2, 0, 1, 0.02, 0.9, True, name)
            n, acc, fb, empty = class_counts(cls)
            print("%s: %d surface pixels, %.1f %% accepted, %.1f %% fallback, %d empty" % (name, n, 100.0 * acc / n, 100.0 * fb / n, empty))
            assert acc >= 0.1 * n and fb >= 0.1 * n and (empty >= 1 or name != "soup_52x44")


def _camera(flat, away=False):
    pts = flat.tri_verts.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    c, d = 0.5 * (lo + hi), hi - lo
    eye = c + np.array([0.1, 0.2, 1.2]) * d
    return eye.tolist(), ((eye + (eye - c)) if away else c).tolist()


@pytest.mark.parametrize("w,h,away", [(1, 1, False), (7, 3, False), (40, 17, True)])
def test_upsample_small_images_and_an_image_of_misses(trx, frames, w, h, away):
    sc = frames("soup_52x44")[0]
    eye, look = _camera(sc.flat, away)
    view = trx.view_from_camera(eye, look, 60.0, w, h)
    fr = Frame(trx, sc, view, w, h, RADIUS["soup_52x44"]).host(trx)
    s = surface(fr.prim)
    assert (not s.any()) if away else (s.any() or w * h < 8)
    for stride, phase in ((1, 0), (2, 3), (3, 4), (4, 0), (4, 15)):
        d_lo = fr.sparse(sc, stride, phase)
        _torch().cuda.synchronize()
        lo = d_lo.cpu().numpy()
        assert (lo == sparse_counts(fr.cnt, w, h, stride, phase)).all()
        for r in (0, 1, 2):
            for attr in (True, False):
                got, _ = _check_upsample(sc, fr, d_lo, lo, stride, phase, r, 0.02, 0.9, attr, "%dx%d" % (w, h))
                if away:
                    assert not got.view(np.uint32).any()


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (70, 19)])
def test_upsample_on_hand_made_records(trx, frames, w, h):
    """Sizes of one pixel, less than a tile, and one pixel past a tile in both directions (32 x 8 tiles), widths and heights
    that are no multiples of the stride, denser in edges than a traced frame: every class next to every tile border."""
    sc = frames("soup_52x44")[0]
    fr = Synthetic(trx, w, h, 5 + w)
    seen = set()
    for stride in (1, 2, 3, 4):
        for phase in sorted({0, stride * stride - 1, (stride * stride) // 2}):
            lo = sparse_counts(fr.cnt, w, h, stride, phase)
            lo[lo == NO_SURFACE] = 200 + stride     # (a cell without a surface: its count is never looked at)
            d_lo = _dev(lo)
            for r in (0, 1, 2):
                for attr in (True, False):
                    for tol, cos in ((0.02, 0.9), (INF, -1.0), (0.0, 1.0), (0.5, 0.0)):
                        _, cls = _check_upsample(sc, fr, d_lo, lo, stride, phase, r, tol, cos, attr, "hand-made %dx%d" % (w, h))
                        seen |= set(np.unique(cls).tolist())
    if w * h > 100:
        assert {ACCEPTED, FALLBACK, EMPTY} <= seen
    fr = Synthetic(trx, w, h, 9, misses=True)
    lo = sparse_counts(fr.cnt, w, h, 2, 1)
    got, _ = _check_upsample(sc, fr, _dev(lo), lo, 2, 1, 2, INF, -1.0, True, "misses %dx%d" % (w, h))
    assert not got.view(np.uint32).any()


def test_upsample_refusals_leave_the_output_untouched(trx, frames):
    from tray_racing_amd import _lib as L
    sc, view, w, h, fr = frames("soup_52x44")
    lib = sc._lib
    d_out = _buf(w * h * 4)
    d_lo = fr.sparse(sc, 2, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def up(s=2, phase=0, n=N, r=1, tol=0.02, cos=0.9, prim=p(fr.d_prim), lo=p(d_lo), out=p(d_out), ww=w):
        return lib.trx_ao_upsample_dev(sc.handle, ww, h, s, phase, prim, p(fr.d_attr), lo, n, r, tol, cos, out, None)

    for kw in ({"s": 0}, {"s": 5}, {"phase": 4}, {"r": 3}, {"n": 0}, {"n": 65}, {"tol": -0.01}, {"tol": float("nan")}, {"cos": float("nan")},
               {"prim": None}, {"lo": None}, {"ww": 0}):
        assert up(**kw) == L.TRX_ERR_INVALID, kw
    assert up(out=None) == L.TRX_ERR_INVALID
    _torch().cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    host = np.full((h, w, 4), FILL, dtype=np.uint8)
    for kw in ({"n": 0}, {"n": 65}, {"radius": 0.0}, {"s": 0}, {"s": 5}, {"phase": 4}, {"r": 3}, {"tol": -1.0}, {"cos": float("nan")}, {"sem": 8}):
        a = dict(n=N, radius=INF, s=2, phase=0, r=1, tol=0.02, cos=0.9, sem=SEM)
        a.update(kw)
        rc = lib.trx_render_image_sparse(sc.handle, C.byref(view), w, h, a["sem"], 0, a["n"], EPS, a["radius"], a["s"], a["phase"], a["r"],
                                         a["tol"], a["cos"], host.ctypes.data_as(C.c_void_p), None)
        assert rc == L.TRX_ERR_INVALID, kw
    assert (host == FILL).all()
    assert up() == 0
    _torch().cuda.synchronize()
    assert (d_out.cpu().numpy() != FILL).any()
    sc.check()


# ---- 3. the host form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_render_image_sparse_is_the_composition_of_the_device_calls(trx, frames, name):
    sc, view, w, h, fr = frames(name)
    for stride, phase, r in ((2, 0, 1), (2, 3, 2), (3, 8, 1), (4, 5, 0), (1, 0, 2)):
        d_lo = fr.sparse(sc, stride, phase)
        d_term = _upsample(sc, fr, d_lo, stride, phase, r, 0.02, 0.9, True)
        d_rgba = _buf(w * h * 4)
        sc.shade_ao_term_dev(d_term.data_ptr(), w * h, d_rgba.data_ptr())
        _torch().cuda.synchronize()
        img, ms = sc.render_image_sparse(view, w, h, N, stride, ao_phase=phase, upsample_radius=r, sem=SEM, frame0=0, ao_eps=EPS,
                                         ao_radius=RADIUS[name], depth_tol=0.02, normal_cos=0.9)
        assert img.shape == (h, w, 4) and ms > 0
        assert (img.reshape(-1, 4) == d_rgba.cpu().numpy().reshape(-1, 4)).all(), (name, stride, phase, r)
        lo = sparse_counts(fr.cnt, w, h, stride, phase)
        assert (img.reshape(-1, 4) == shade_term(ao_upsample(fr.prim, fr.attr["normal"], lo, w, h, stride, phase, N, r, 0.02, 0.9))).all()
        if stride == 1:
            dense, _ = sc.render_image(view, w, h, sem=SEM, frame0=0, n_samples=N, ao_eps=EPS, ao_radius=RADIUS[name], filter_radius=r,
                                       depth_tol=0.02, normal_cos=0.9)
            assert (img == dense).all(), "stride 1 is not trx_render_image's frame"
        else:
            assert np.unique(img[..., 0]).size > 2
    sc.check()


# ---- 4. ordering with refit -------------------------------------------------------------------------------------------

def test_sparse_chain_keeps_its_place_before_a_refit(trx):
    """A frame's whole sparse chain - trace, attributes, sparse visibility, upsample, shade - enqueued on a busy stream, then
    at once a refit: the refit waits for every launch of the chain, the image is the old geometry's."""
    torch = _torch()
    flat, view, w, h = _golden_scene(trx, "soup_52x44")
    sc = trx.Scene(flat)
    v = flat.tri_verts
    size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
    moved = (v + np.random.default_rng(71).normal(scale=2e-2 * size, size=v.shape)).astype(np.float32)

    def chain(stream=0):
        fr = Frame(trx, sc, view, w, h, RADIUS["soup_52x44"], stream=stream, dense=False)
        d_lo = fr.sparse(sc, 2, 1, stream=stream)
        d_term = _upsample(sc, fr, d_lo, 2, 1, 1, 0.02, 0.9, True, stream=stream)
        d_rgba = _buf(w * h * 4)
        sc.shade_ao_term_dev(d_term.data_ptr(), w * h, d_rgba.data_ptr(), stream=stream)
        return fr, d_lo, d_term, d_rgba

    try:
        old = chain()
        torch.cuda.synchronize()
        old = [t.cpu().numpy() for t in old[1:]]
        s = torch.cuda.Stream()
        big = random_rays(trx, flat, 2 * 1024 * 1024, 72, zero_dirs=False)
        d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), sem=SEM, stream=s.cuda_stream)
            got = chain(stream=s.cuda_stream)
        sc.refit(moved)
        s.synchronize()
        for what, g, o in zip(("low grid", "term", "image"), got[1:], old):
            assert (g.cpu().numpy() == o).all(), "%s: the chain saw the refit's geometry" % what
        new = chain()
        torch.cuda.synchronize()
        assert (new[3].cpu().numpy() != old[2]).sum() > 100, "the refit changed nothing"
        sc.check()
    finally:
        sc.close()
