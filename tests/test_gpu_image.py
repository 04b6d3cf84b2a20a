"""The frame's image on the GPU, bit for bit against the numpy twin (tests/image_twin.py): the edge-aware AO filter
(trx_ao_filter_dev) for every radius / tolerance / cosine class, the three shades (trx_shade_*_dev) in both layouts, and
trx_render_image against the composition of the device calls - fed the library's own primary, attribute and AO records
(held to the oracle and their twins by test_gpu_parity.py, test_gpu_hit_attr.py and test_gpu_ao_visibility.py) on the
committed fixtures soup_52x44 (44 rows: the filter's 32 x 8 tiles and their halo end inside the image's last tiles) and
cornell_tlas_48 (two-level).  No pixel is left out of any comparison."""
import ctypes as C
import os

import numpy as np
import pytest

from ao_visibility_twin import record_map
from helpers import random_rays
from image_twin import AO_NO_SURFACE, TERM_DTYPE, ao_filter, shade_counts, shade_reference, shade_term, surface

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
SEM, N, EPS = 3, 4, 0.01
RADIUS = {"soup_52x44": 0.8, "cornell_tlas_48": 1.4}
FILL = 0xA5
WHOLE = (0, 1, 0)


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


def _host(t, dtype, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n * np.dtype(dtype).itemsize]).view(dtype)


class Frame:
    """The records of one frame as the library's passes leave them on the device, for `shard` = (index, count, layout)."""

    def __init__(self, trx, sc, view, w, h, radius, shard=WHOLE, stream=0, attr=True):
        from tray_racing_amd import _lib as L
        self.w, self.h, self.shard = w, h, shard
        self.pix, self.rec, self.n = record_map(w, h, shard)
        n = self.n
        self.d_prim, self.d_inst, self.d_ao = _buf(n * 8), _buf(n * 4), _buf(n * 8)
        self.d_attr, self.d_cnt = _buf(n * 24), _buf(n)
        S, p = L.Shard(shard[0], shard[1], shard[2], 0), (lambda t: C.c_void_p(t.data_ptr()))
        st = C.c_void_p(stream)
        lib = sc._lib
        L.check(lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, S, SEM, p(self.d_prim), p(self.d_inst), st))
        L.check(lib.trx_trace_ao_inst_dev(sc.handle, C.byref(view), w, h, S, SEM, 0, EPS, p(self.d_prim), p(self.d_inst), p(self.d_ao),
                                          None, st))
        if attr:
            sc.hit_attributes_primary_dev(view, w, h, self.d_prim.data_ptr(), self.d_attr.data_ptr(), d_inst=self.d_inst.data_ptr(),
                                          shard=shard, stream=stream)
        sc.trace_ao_visibility_dev(view, w, h, self.d_prim.data_ptr(), self.d_cnt.data_ptr(), N, radius, sem=SEM, frame0=0,
                                   ao_eps=EPS, d_primary_inst=self.d_inst.data_ptr(), shard=shard, stream=stream)

    def host(self, trx):
        _torch().cuda.synchronize()
        self.prim, self.ao = _host(self.d_prim, trx.HIT_DTYPE), _host(self.d_ao, trx.HIT_DTYPE)
        self.attr, self.cnt = _host(self.d_attr, trx.HIT_ATTR_DTYPE), _host(self.d_cnt, np.uint8, self.n)
        return self


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
    """name -> (scene, view, w, h, the whole-image frame with its host copies): traced once, read by every test."""
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


def _filter(sc, fr, r, tol, cos, attr, n=N, stream=0):
    d_term = _buf(fr.n * 4 + 64)
    sc.ao_filter_dev(fr.w, fr.h, fr.d_prim.data_ptr(), fr.d_cnt.data_ptr(), d_term.data_ptr(), n, r, depth_tol=tol, normal_cos=cos,
                     d_attr=fr.d_attr.data_ptr() if attr else 0, stream=stream)
    return d_term


def _check_filter(trx, sc, fr, r, tol, cos, attr, what):
    d_term = _filter(sc, fr, r, tol, cos, attr)
    _torch().cuda.synchronize()
    raw = d_term.cpu().numpy()
    assert (raw[fr.n * 4:] == FILL).all(), what + ": bytes past the image were written"
    got = raw[:fr.n * 4].view(TERM_DTYPE)
    want = ao_filter(fr.prim, fr.attr["normal"] if attr else None, fr.cnt, fr.w, fr.h, N, r, tol, cos)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s r %d tol %g cos %g attr %d: %d pixels differ (first %s: %s vs %s)" % (
        what, r, tol, cos, attr, bad.size, divmod(int(bad[0]), fr.w)[::-1], got[bad[0]], want[bad[0]])
    return got


def _box_sum(fr, r):
    """The plain clipped box sums over the surface pixels: counts and N per surface pixel, by a summed-area table."""
    s = surface(fr.prim).reshape(fr.h, fr.w)
    out = []
    for a in (np.where(s, fr.cnt.reshape(fr.h, fr.w), 0).astype(np.int64), s.astype(np.int64) * N):
        sat = np.zeros((fr.h + 1, fr.w + 1), dtype=np.int64)
        sat[1:, 1:] = a.cumsum(0).cumsum(1)
        y, x = np.mgrid[0:fr.h, 0:fr.w]
        y0, y1, x0, x1 = np.maximum(y - r, 0), np.minimum(y + r, fr.h - 1) + 1, np.maximum(x - r, 0), np.minimum(x + r, fr.w - 1) + 1
        out.append(np.where(s, sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0], 0).reshape(-1))
    return out


# ---- 1. the filter against the twin ---------------------------------------------------------------------------------

@pytest.mark.parametrize("attr", [True, False])
@pytest.mark.parametrize("r", [0, 1, 4])
@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_filter_against_twin(trx, frames, name, r, attr):
    sc, view, w, h, fr = frames(name)
    s = surface(fr.prim)
    assert 0.2 * s.size < s.sum() and (fr.cnt[s] <= N).all() and (fr.cnt[~s] == AO_NO_SURFACE).all()
    for tol in (0.0, 0.02, INF):
        for cos in ((-1.0, 0.9, 1.0) if attr else (0.9,)):
            got = _check_filter(trx, sc, fr, r, tol, cos, attr, name)
            assert not got.view(np.uint32)[~s].any()
            if r == 0:
                assert (got["unoccluded"][s] == fr.cnt[s]).all() and (got["samples"][s] == N).all()
            if tol == INF and (cos == -1.0 or not attr):
                u, n = _box_sum(fr, r)
                assert (got["unoccluded"] == u).all() and (got["samples"] == n).all(), "not the plain box sum"
    if r == 4 and attr:
        # the edge tests do something on these frames: fewer pixels accepted than the box holds, more than the pixel alone
        edge = _check_filter(trx, sc, fr, r, 0.02, 0.9, True, name)["samples"][s].astype(int).sum()
        assert N * s.sum() < edge < _box_sum(fr, r)[1][s].sum()


def _camera(flat, away=False):
    pts = flat.tri_verts.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    c, d = 0.5 * (lo + hi), hi - lo
    eye = c + np.array([0.1, 0.2, 1.2]) * d
    return eye.tolist(), ((eye + (eye - c)) if away else c).tolist()


@pytest.mark.parametrize("w,h,away", [(1, 1, False), (7, 3, False), (40, 17, True)])
def test_filter_small_images_and_an_image_of_misses(trx, frames, w, h, away):
    sc, _, _, _, _ = frames("soup_52x44")
    eye, look = _camera(sc.flat, away)
    view = trx.view_from_camera(eye, look, 60.0, w, h)
    fr = Frame(trx, sc, view, w, h, RADIUS["soup_52x44"]).host(trx)
    s = surface(fr.prim)
    assert (not s.any()) if away else (s.any() or w * h < 8)
    for r in (0, 1, 4):
        for attr in (True, False):
            got = _check_filter(trx, sc, fr, r, 0.02, 0.9, attr, "%dx%d" % (w, h))
            if away:
                assert not got.view(np.uint32).any()
    d_rgba = _buf(fr.n * 4)
    sc.shade_ao_counts_dev(fr.d_cnt.data_ptr(), N, fr.n, d_rgba.data_ptr())
    _torch().cuda.synchronize()
    img = d_rgba.cpu().numpy().reshape(-1, 4)
    assert (img == shade_counts(fr.cnt, N)).all() and (not away or (img == [0, 0, 0, 255]).all())


class Synthetic:
    """Hand-made whole-image records on the device: depth steps, misses of both kinds, three normals, counts 0..N."""

    def __init__(self, trx, w, h, seed):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.n = w, h, w * h
        self.prim = np.zeros(self.n, dtype=trx.HIT_DTYPE)
        self.prim["t"] = rng.choice(np.array([1.0, 1.01, 1.5, INF, 3.4028234663852886e38], dtype=np.float32), self.n, p=[.4, .3, .15, .1, .05])
        self.prim["prim"] = np.where(rng.random(self.n) < 0.08, 0xFFFFFFFF, rng.integers(0, 1000, self.n)).astype(np.uint32)
        self.attr = np.zeros(self.n, dtype=trx.HIT_ATTR_DTYPE)
        self.attr["normal"] = np.array([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]], dtype=np.float32)[rng.integers(0, 3, self.n)]
        self.cnt = np.where(surface(self.prim), rng.integers(0, N + 1, self.n), AO_NO_SURFACE).astype(np.uint8)
        self.d_prim, self.d_attr, self.d_cnt = _dev(self.prim), _dev(self.attr), _dev(self.cnt)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (70, 19)])
def test_filter_on_hand_made_records(trx, frames, w, h):
    """Sizes of one pixel, less than a tile, and one pixel past a tile in both directions (32 x 8 tiles), denser in edges
    than a traced frame: every class of pixel and neighbour next to every tile border."""
    sc = frames("soup_52x44")[0]
    fr = Synthetic(trx, w, h, 5 + w)
    for r in (0, 1, 2, 4):
        for attr in (True, False):
            for tol, cos in ((0.02, 0.9), (INF, -1.0), (0.0, 1.0), (0.5, 0.0)):
                _check_filter(trx, sc, fr, r, tol, cos, attr, "hand-made %dx%d" % (w, h))


# ---- 2. the shades against the twin ----------------------------------------------------------------------------------

def _shade_all(sc, fr, d_term, stream=0):
    """The three shades of a frame's records into buffers with 64 spare bytes: (reference, counts, term) tensors."""
    out = [_buf(fr.n * 4 + 64) for _ in range(3)]
    sc.shade_reference_dev(fr.d_prim.data_ptr(), fr.d_ao.data_ptr(), fr.n, out[0].data_ptr(), stream=stream)
    sc.shade_ao_counts_dev(fr.d_cnt.data_ptr(), N, fr.n, out[1].data_ptr(), stream=stream)
    sc.shade_ao_term_dev(d_term.data_ptr(), fr.n, out[2].data_ptr(), stream=stream)
    return out


@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_shades_against_twin_in_both_layouts(trx, frames, name):
    sc, view, w, h, whole = frames(name)
    term = ao_filter(whole.prim, whole.attr["normal"], whole.cnt, w, h, N, 2, 0.02, 0.9)
    # image layout; and shard 1 of 3 in TRX_LAYOUT_SHARD: compact records, the last tiles' records outside the image never
    # written by the passes (they keep the fill, and are shaded like any other bytes)
    shard = Frame(trx, sc, view, w, h, RADIUS[name], shard=(1, 3, 1), attr=False).host(trx)
    shard_term = np.frombuffer(bytes([FILL]) * (shard.n * 4), dtype=TERM_DTYPE).copy()
    shard_term[shard.rec] = term[shard.pix]
    for fr, t in ((whole, term), (shard, shard_term)):
        outs = _shade_all(sc, fr, _dev(t))
        _torch().cuda.synchronize()
        wants = (shade_reference(fr.prim, fr.ao), shade_counts(fr.cnt, N), shade_term(t))
        for mode, d, want in zip(("reference", "counts", "term"), outs, wants):
            raw = d.cpu().numpy()
            assert (raw[fr.n * 4:] == FILL).all(), "%s %s: bytes past n_records * 4 were written" % (name, mode)
            got = raw[:fr.n * 4].reshape(-1, 4)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, "%s %s layout %d: %d records differ (first %d: %s vs %s)" % (
                name, mode, fr.shard[2], bad.size, bad[0], got[bad[0]], want[bad[0]])
            assert (got[:, 3] == 255).all() and np.unique(got[:, 0]).size > 2
    # the shard's records are the image's
    assert (shard.cnt[shard.rec] == whole.cnt[shard.pix]).all()
    # the reference mode is the command line's image: the save_png arithmetic over trx_trace_primary_ao's records
    prim, ao, _ = sc.trace_primary_ao(view, w, h, sem=SEM, frame=0, ao_eps=EPS)
    d_rgba = _buf(w * h * 4)
    sc.shade_reference_dev(whole.d_prim.data_ptr(), whole.d_ao.data_ptr(), w * h, d_rgba.data_ptr())
    _torch().cuda.synchronize()
    assert (d_rgba.cpu().numpy().reshape(-1, 4) == shade_reference(prim, ao)).all()
    # zero records: nothing to do, no error
    sc.shade_ao_term_dev(0, 0, 0)


# ---- 3. trx_render_image ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_render_image_is_the_composition_of_the_device_calls(trx, frames, name):
    sc, view, w, h, fr = frames(name)
    radius = RADIUS[name]
    # filtered: the attribute pass, the filter with normals, the term shade
    d_term = _filter(sc, fr, 2, 0.02, 0.9, True)
    d_rgba = _buf(w * h * 4)
    sc.shade_ao_term_dev(d_term.data_ptr(), w * h, d_rgba.data_ptr())
    _torch().cuda.synchronize()
    img, ms = sc.render_image(view, w, h, sem=SEM, frame0=0, n_samples=N, ao_eps=EPS, ao_radius=radius, filter_radius=2,
                              depth_tol=0.02, normal_cos=0.9)
    assert img.shape == (h, w, 4) and ms > 0
    assert (img.reshape(-1, 4) == d_rgba.cpu().numpy().reshape(-1, 4)).all()
    assert (img.reshape(-1, 4) == shade_term(ao_filter(fr.prim, fr.attr["normal"], fr.cnt, w, h, N, 2, 0.02, 0.9))).all()
    # unfiltered: the twin's image of the host form's counts
    counts, _ = sc.trace_ao_visibility(view, w, h, N, radius, sem=SEM, frame0=0, ao_eps=EPS)
    img, _ = sc.render_image(view, w, h, sem=SEM, frame0=0, n_samples=N, ao_eps=EPS, ao_radius=radius, filter_radius=0)
    assert (img.reshape(-1, 4) == shade_counts(counts, N)).all() and (counts == fr.cnt).all()
    # no samples: the reference's image of the host form's records
    prim, ao, _ = sc.trace_primary_ao(view, w, h, sem=SEM, frame=0, ao_eps=EPS)
    img, _ = sc.render_image(view, w, h, sem=SEM, frame0=0, n_samples=0, ao_eps=EPS)
    assert (img.reshape(-1, 4) == shade_reference(prim, ao)).all()
    sc.check()


# ---- 4. refused calls leave the output untouched ---------------------------------------------------------------------

def test_refused_calls_leave_the_output_untouched(trx, frames):
    from tray_racing_amd import _lib as L
    sc, view, w, h, fr = frames("soup_52x44")
    lib = sc._lib
    d_out = _buf(w * h * 4)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def filt(n=N, r=1, tol=0.02, cos=0.9, prim=p(fr.d_prim), cnt=p(fr.d_cnt), out=p(d_out), ww=w):
        return lib.trx_ao_filter_dev(sc.handle, ww, h, prim, p(fr.d_attr), cnt, n, r, tol, cos, out, None)

    for kw in ({"r": 5}, {"n": 0}, {"n": 65}, {"tol": -0.01}, {"tol": float("nan")}, {"cos": float("nan")}, {"prim": None},
               {"cnt": None}, {"ww": 0}):
        assert filt(**kw) == L.TRX_ERR_INVALID, kw
    assert filt(out=None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_ao_counts_dev(sc.handle, p(fr.d_cnt), 0, w * h, p(d_out), None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_ao_counts_dev(sc.handle, p(fr.d_cnt), 65, w * h, p(d_out), None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_ao_counts_dev(sc.handle, None, N, w * h, p(d_out), None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_reference_dev(sc.handle, p(fr.d_prim), None, w * h, p(d_out), None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_ao_term_dev(sc.handle, None, w * h, p(d_out), None) == L.TRX_ERR_INVALID
    assert lib.trx_shade_ao_term_dev(sc.handle, p(fr.d_cnt), w * h, C.c_void_p(d_out.data_ptr() + 1), None) == L.TRX_ERR_INVALID
    _torch().cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    host = np.full((h, w, 4), FILL, dtype=np.uint8)
    for kw in ({"n_samples": 65}, {"n_samples": N, "ao_radius": 0.0}, {"n_samples": N, "filter_radius": 5},
               {"n_samples": N, "filter_radius": 1, "depth_tol": -1.0}, {"n_samples": N, "filter_radius": 1, "normal_cos": float("nan")}):
        a = dict(n_samples=0, ao_radius=INF, filter_radius=0, depth_tol=0.02, normal_cos=0.9)
        a.update(kw)
        rc = lib.trx_render_image(sc.handle, C.byref(view), w, h, SEM, 0, a["n_samples"], EPS, a["ao_radius"], a["filter_radius"],
                                  a["depth_tol"], a["normal_cos"], host.ctypes.data_as(C.c_void_p), None)
        assert rc == L.TRX_ERR_INVALID, kw
    assert (host == FILL).all()
    sc.check()


# ---- 5. ordering with refit -------------------------------------------------------------------------------------------

def test_image_passes_keep_their_place_before_a_refit(trx):
    """A frame's whole chain - trace, attributes, visibility, filter, shade - enqueued on a busy stream, then at once a refit:
    the refit waits for every launch of the chain, the image is the old geometry's."""
    torch = _torch()
    flat, view, w, h = _golden_scene(trx, "soup_52x44")
    sc = trx.Scene(flat)
    v = flat.tri_verts
    size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
    moved = (v + np.random.default_rng(71).normal(scale=2e-2 * size, size=v.shape)).astype(np.float32)

    def chain(stream=0):
        fr = Frame(trx, sc, view, w, h, RADIUS["soup_52x44"], stream=stream)
        d_term = _filter(sc, fr, 2, 0.02, 0.9, True, stream=stream)
        return fr, d_term, _shade_all(sc, fr, d_term, stream=stream)

    try:
        _, _, old = chain()
        torch.cuda.synchronize()
        old = [t.cpu().numpy() for t in old]
        s = torch.cuda.Stream()
        big = random_rays(trx, flat, 2 * 1024 * 1024, 72, zero_dirs=False)
        d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), sem=SEM, stream=s.cuda_stream)
            fr, d_term, got = chain(stream=s.cuda_stream)
        sc.refit(moved)
        s.synchronize()
        for mode, g, o in zip(("reference", "counts", "term"), got, old):
            assert (g.cpu().numpy() == o).all(), "%s: the chain saw the refit's geometry" % mode
        _, _, new = chain()
        torch.cuda.synchronize()
        assert all((n.cpu().numpy() != o).sum() > 100 for n, o in zip(new, old)), "the refit changed nothing"
        sc.check()
    finally:
        sc.close()
