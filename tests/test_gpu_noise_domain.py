"""The device's noise-driven ray generators over the whole hash domain, bit for bit against the oracle.

Every stochastic pass draws u1 = hash_noise(px, py, seed), u2 = hash_noise(px, py, seed + 1024).  A frame test visits the hash
values its few seeds happen to produce; here a pixel is GIVEN the hash value (tests/noise_domain.py: seed_for inverts uhash):
u == 0, u == 1.0f, both sides of the small-angle branch, of the reduction switch and of every quadrant switch of the sine /
cosine, and seeds whose sums wrap at 2^32 - through every entry point that draws the noise: trx_ao_rays_dev, the closest-hit
AO passes, the sparse and dense visibility passes, the rect light's sample and the bounce.  The dense leg then holds the
device's sine / cosine to the oracle's on 2^19 distinct arguments.  tests/test_noise_domain.py asserts, without a GPU, what
each target reaches and that the oracle's rays there have the properties of the definition.

Every comparison is over the whole buffer, in bits; every output buffer is pre-filled with a sentinel.  Every step that runs
on the GPU sits under a time limit of its own (`limit`)."""
import ctypes as C

import numpy as np
import pytest

import indirect_sparse_twin as IST
import indirect_twin as IT
import light_twin as LT
import noise_domain as ND
from ao_sparse_twin import lo_size, sparse_counts
from ao_visibility_twin import INVALID, NO_SURFACE, stored_tmax, visibility_counts
from test_gpu_ao_visibility import _visibility, make_case
from test_gpu_indirect import ALBEDO, UNIT as BOUNCE_UNIT, Gi, _device_bounce
from test_gpu_light import EPS, Lit, _buf, _dev, _sync, _torch, limit

pytestmark = pytest.mark.gpu
INF = float("inf")
M32 = 0xFFFFFFFF
SENTINEL = 0xA5A5A5A5
GOLDEN_CASES = ("cornell_64", "cornell_tlas_48")
POINT_LIGHT = LT.Light(LT.POINT, (0.0, 1.8, 0.0), intensity=1.5)
LIGHTS = [POINT_LIGHT, LT.RECT_CASE]                       # the rect light at index k = 1
# (target, as the second noise): the rect light's point on the rectangle's far and near edges
RECT_TARGETS = (("0", False), ("last-1.0", False), ("0", True), ("first-1.0", True))


def _noise(orc, px, py, seed, second):
    return np.float32(orc.load().orc_hash_noise(px, py, (seed + (1024 if second else 0)) & M32))


def _claimed(orc, px, py, seed, tname, second):
    """The oracle's u at the target pixel is the target's."""
    assert _noise(orc, px, py, seed, second).tobytes() == ND.u_of(ND.TARGETS[tname]).tobytes(), (tname, px, py, second)


def _differences(got, want, w, what):
    """'' or one line naming the records (8 words each) that differ."""
    bad = np.flatnonzero((got != want).any(1))
    if bad.size == 0:
        return ""
    i = int(bad[0])
    return "%s: %d of %d records differ, first %d (pixel %d, %d): %s != %s" % (
        what, bad.size, got.shape[0], i, i % w, i // w, ["%08x" % x for x in got[i]], ["%08x" % x for x in want[i]])


class Domain:
    """The hand-made scenes on the device and on the oracle, their view and their hand-made records."""

    def __init__(self, trx, orc):
        self.trx, self.orc = trx, orc
        eye, look, fov = ND.CAMERA
        self.view = trx.view_from_camera(eye, look, fov, ND.W, ND.H)
        self.oview = orc.view_from_bytes(bytes(self.view))
        self.dense_view = trx.view_from_camera(eye, look, fov, ND.DENSE, ND.DENSE)
        flat = ND.single_level(trx)
        flat2, self.pairs = ND.two_level(trx)
        self.scenes = {"single": trx.Scene(flat), "two-level": trx.Scene(flat2)}
        # the oracle takes normals to world space through the world-to-object rows the kernels use
        self.oscenes = {"single": orc.Scene.from_flat(flat),
                        "two-level": orc.Scene(flat2.nodes, flat2.tri_verts, flat2.instance_offsets, flat2.tlas_start,
                                               instance_w2o=self.scenes["two-level"].instance_world_to_object())}
        self.n_tris = flat.n_tris

    def records(self, name, w, h, shift=0):
        """(records, instance ids or None, their device copies)."""
        rec, inst = ND.records(self.orc.HIT_DTYPE, w, h, n_tris=self.n_tris, pairs=self.pairs if name == "two-level" else None, shift=shift)
        return rec, inst, _dev(rec), None if inst is None else _dev(inst)

    def device_rays(self, name, view, w, h, d_prim, d_inst, frame, radius, eps):
        """trx_ao_rays_dev's records [w * h, 8] as words; a sentinel record on either side of the buffer must survive."""
        torch = _torch()
        n = w * h
        d_rays = torch.full(((n + 2) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        _sync()
        with limit():
            self.scenes[name].ao_rays_dev(view, w, h, d_prim.data_ptr(), d_rays.data_ptr() + 32, radius, frame=frame, ao_eps=eps,
                                          d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0)
            torch.cuda.synchronize()
            self.scenes[name].check()
        got = d_rays.cpu().numpy().view(np.uint32).reshape(n + 2, 8)
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "a guard record was written"
        return got[1:-1]

    def oracle_rays(self, name, oview, w, h, rec, inst, frame, radius, eps, threads=4):
        return self.oscenes[name].ao_rays(oview, w, h, rec, inst, frame=frame, ao_eps=eps, tmax=float(stored_tmax(radius)),
                                          threads=threads).view(np.uint32).reshape(-1, 8)

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def dom(trx, orc):
    d = Domain(trx, orc)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases(trx, orc):
    """The golden cases of tests/test_gpu_ao_visibility.py (real primary hits), with the light and the indirect twins' needs."""
    made, lit, gis = {}, {}, {}

    def get(name):
        case = make_case(trx, orc, made, name)
        if name not in lit:
            lit[name], gis[name] = Lit(case), Gi(case)
        return case, lit[name], gis[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


def _surface_pixel(prim, w, k):
    """A surface pixel, another one (in another lane of its tile) for every k."""
    surf = np.flatnonzero((prim["t"] < 3.4028234663852886e38) & (prim["prim"] != INVALID))
    i = int(surf[(k * 131 + 29) % surf.size])
    return i % w, i // w, i


def _oracle_primary(case, sem, prim, inst):
    """The device's primary records are the oracle's (so a pixel picked from them is picked by the oracle)."""
    want, want_inst, _ = case.osc.trace_primary_inst(case.oview, case.w, case.h, sem=sem)
    assert prim.tobytes() == want.tobytes() and (inst == want_inst).all(), case.name


# ---- a. trx_ao_rays_dev at every target, as u1 and as u2 ---------------------------------------------------------------------

@pytest.mark.parametrize("second", [False, True], ids=["u1", "u2"])
@pytest.mark.parametrize("name", ["single", "two-level"])
def test_ao_rays_at_every_target(trx, orc, dom, name, second):
    w, h = ND.W, ND.H
    rec, inst, d_prim, d_inst = dom.records(name, w, h)
    failures = []
    for k, (tname, target) in enumerate(ND.TARGETS.items()):
        px, py = ND.target_pixel(k + 3 * second)
        seed = ND.seed_for(px, py, target, second)
        i = py * w + px
        assert rec["t"][i] < 3.4028234663852886e38 and rec["prim"][i] != INVALID           # the target pixel is a surface
        _claimed(orc, px, py, seed, tname, second)
        radius, eps = (INF, 0.01) if k % 2 == 0 else (1.5, 0.0001)
        got = dom.device_rays(name, dom.view, w, h, d_prim, d_inst, seed, radius, eps)
        want = dom.oracle_rays(name, dom.oview, w, h, rec, inst, seed, radius, eps)
        assert not (want == SENTINEL).all(1).any()
        diff = _differences(got, want, w, "%s %s as %s (hash 0x%08X, seed 0x%08X, target pixel %d, %d)" % (
            name, tname, "u2" if second else "u1", target, seed, px, py))
        if diff:
            failures.append(diff + (" - the target pixel among them" if (got[i] != want[i]).any() else ""))
    print("trx_ao_rays_dev %s: %d targets as %s" % (name, len(ND.TARGETS), "u2" if second else "u1"))
    assert not failures, "\n".join(failures)


# ---- b. seeds whose sums wrap ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two-level"])
def test_ao_rays_with_wrapping_seeds(trx, orc, dom, name):
    """frame + 1024 wraps at 0xFFFFFFFF (and (py << 11) + frame in every row but the first); at 0xFFFFFC00 it is exactly 2^32;
    at 0xFFFFFBFF it is the last sum that does not wrap."""
    w, h = ND.W, ND.H
    rec, inst, d_prim, d_inst = dom.records(name, w, h, shift=5)
    failures = []
    for frame in (0xFFFFFFFF, 0xFFFFFC00, 0xFFFFFBFF):
        got = dom.device_rays(name, dom.view, w, h, d_prim, d_inst, frame, INF, 0.01)
        want = dom.oracle_rays(name, dom.oview, w, h, rec, inst, frame, INF, 0.01)
        failures.append(_differences(got, want, w, "%s frame 0x%08X" % (name, frame)))
        # the second noise of this frame is the first noise of frame + 1024 mod 2^32: the sum wrapped, it did not saturate
        assert (ND.image_hashes(w, h, frame, second=True) == ND.image_hashes(w, h, (frame + 1024) & M32)).all()
    assert not any(failures), "\n".join(f for f in failures if f)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_visibility_with_a_wrapping_frame0(trx, orc, cases, name):
    """frame0 = 0xFFFFFFFC, 8 samples: the seeds are 0xFFFFFFFC .. 0xFFFFFFFF, 0 .. 3."""
    case, _, _ = cases(name)
    for sem in (0, 3):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem)
        with limit():
            got = _visibility(case, d_prim, d_inst, 8, case.radius, sem, (0, 1, 0), frame0=0xFFFFFFFC)
        want = visibility_counts(orc, case.osc, case.oview, case.w, case.h, prim, inst, sem, 0xFFFFFFFC, 8, 0.01, case.radius)
        assert (got == want).all(), "%s sem %d: %d bytes differ" % (name, sem, (got != want).sum())
        # seeds taken mod 2^32: the last four samples are the seeds 0 .. 3
        top = visibility_counts(orc, case.osc, case.oview, case.w, case.h, prim, inst, sem, 0xFFFFFFFC, 4, 0.01, case.radius)
        low = visibility_counts(orc, case.osc, case.oview, case.w, case.h, prim, inst, sem, 0, 4, 0.01, case.radius)
        surf = want != NO_SURFACE
        assert (want[surf] == top[surf] + low[surf]).all() and 0 < low[surf].sum() < 4 * surf.sum()


def _inst_fill(case):
    """The sentinel of an instance-id buffer: single-level scenes write no instance ids, so theirs starts as the id of a miss."""
    return 0xEE if case.osc.inst.size else 0xFF


def _ao_inst_dev(case, d_prim, d_inst, sem, frame, fill=0xEE):
    """trx_trace_ao_inst_dev: (hit records, instance ids) of one AO pass."""
    from tray_racing_amd import _lib as L
    n = case.w * case.h
    d_ao, d_ai = _buf(n * 8, fill), _buf(n * 4, _inst_fill(case))
    _sync()
    with limit():
        L.check(case.sc._lib.trx_trace_ao_inst_dev(case.sc.handle, C.byref(case.view), case.w, case.h, L.Shard(0, 1, 0, 0), sem, frame, 0.01,
                                                   C.c_void_p(d_prim.data_ptr()), C.c_void_p(d_inst.data_ptr()), C.c_void_p(d_ao.data_ptr()),
                                                   C.c_void_p(d_ai.data_ptr()), C.c_void_p(0)))
        _torch().cuda.synchronize()
        case.sc.check()
    return d_ao.cpu().numpy().view(case.orc.HIT_DTYPE), d_ai.cpu().numpy().view(np.uint32)


def _ao_batch_dev(case, d_prim, d_inst, sem, frame0, n_frames, fill=0xEE):
    """trx_trace_ao_batch_dev: ([n_frames, w * h] hit records, instance ids)."""
    n = case.w * case.h
    d_ao, d_ai = _buf(n_frames * n * 8, fill), _buf(n_frames * n * 4, _inst_fill(case))
    _sync()
    with limit():
        case.sc.trace_ao_batch_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_ao.data_ptr(), n, n_frames, sem=sem, frame0=frame0,
                                   d_primary_inst=d_inst.data_ptr(), d_ao_inst=d_ai.data_ptr())
        _torch().cuda.synchronize()
        case.sc.check()
    return d_ao.cpu().numpy().view(case.orc.HIT_DTYPE).reshape(n_frames, n), d_ai.cpu().numpy().view(np.uint32).reshape(n_frames, n)


def _oracle_ao(case, prim, inst, sem, frame):
    ao, ai, _ = case.osc.trace_ao_inst(case.oview, case.w, case.h, prim, inst, sem=sem, frame=frame & M32, ao_eps=0.01, threads=4)
    return ao, ai


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_ao_batch_with_a_wrapping_frame0(trx, orc, cases, name):
    """frame0 = 0xFFFFFFFD, 8 frames: equal to eight separate launches under the seeds mod 2^32, and to the oracle."""
    case, _, _ = cases(name)
    for sem in (0, 3):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem)
        ao, ai = _ao_batch_dev(case, d_prim, d_inst, sem, 0xFFFFFFFD, 8)
        for f in range(8):
            seed = (0xFFFFFFFD + f) & M32
            one, one_i = _ao_inst_dev(case, d_prim, d_inst, sem, seed)
            want, want_i = _oracle_ao(case, prim, inst, sem, seed)
            what = "%s sem %d frame %d (seed 0x%08X)" % (name, sem, f, seed)
            assert ao[f].tobytes() == one.tobytes() and (ai[f] == one_i).all(), what + ": the batch differs from the single launch"
            assert one.tobytes() == want.tobytes() and (one_i == want_i).all(), what + ": the launch differs from the oracle"
        assert ao[3].tobytes() != ao[4].tobytes()


# ---- c. the closest-hit AO passes ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("second", [False, True], ids=["u1", "u2"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_closest_hit_ao_passes_at_the_targets(trx, orc, cases, name, second):
    """trx_trace_ao_inst_dev, trx_trace_frame_dev and trx_trace_ao_batch_dev (the target seed at frame 5 of 8) against
    orc_trace_ao_inst, the target given to a surface pixel of a real primary pass."""
    case, _, _ = cases(name)
    w, h, n = case.w, case.h, case.w * case.h
    failures = []
    for sem in (0, 3):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem)
        _oracle_primary(case, sem, prim, inst)
        for k, tname in enumerate(ND.CORE_TARGETS):
            px, py, i = _surface_pixel(prim, w, 2 * k + second + sem)
            seed = ND.seed_for(px, py, ND.TARGETS[tname], second)
            _claimed(orc, px, py, seed, tname, second)
            what = "%s sem %d %s as %s (seed 0x%08X, pixel %d, %d)" % (name, sem, tname, "u2" if second else "u1", seed, px, py)
            want, want_i = _oracle_ao(case, prim, inst, sem, seed)
            got, got_i = _ao_inst_dev(case, d_prim, d_inst, sem, seed)
            if got.tobytes() != want.tobytes() or (got_i != want_i).any():
                bad = np.flatnonzero((got["t"].view(np.uint32) != want["t"].view(np.uint32)) | (got["prim"] != want["prim"]) | (got_i != want_i))
                failures.append("%s: trx_trace_ao_inst_dev differs at records %s%s" % (what, bad[:6], ", the target pixel among them" if i in bad else ""))
            # the fused frame: primary and AO in one launch
            d_p2, d_pi2, d_ao, d_ai = _buf(n * 8, 0xEE), _buf(n * 4, _inst_fill(case)), _buf(n * 8, 0xEE), _buf(n * 4, _inst_fill(case))
            _sync()
            with limit():
                case.sc.trace_frame_dev(case.view, w, h, d_p2.data_ptr(), d_ao.data_ptr(), sem=sem, frame=seed, ao_eps=0.01,
                                        d_primary_inst=d_pi2.data_ptr(), d_ao_inst=d_ai.data_ptr())
                _torch().cuda.synchronize()
                case.sc.check()
            assert d_p2.cpu().numpy().tobytes() == prim.tobytes() and (d_pi2.cpu().numpy().view(np.uint32) == inst).all(), what
            fused, fused_i = d_ao.cpu().numpy().view(orc.HIT_DTYPE), d_ai.cpu().numpy().view(np.uint32)
            if fused.tobytes() != want.tobytes() or (fused_i != want_i).any():
                failures.append("%s: trx_trace_frame_dev differs in %d records" % (what, (fused.view(np.uint64) != want.view(np.uint64)).sum()))
            batch, batch_i = _ao_batch_dev(case, d_prim, d_inst, sem, (seed - 5) & M32, 8)
            if batch[5].tobytes() != want.tobytes() or (batch_i[5] != want_i).any():
                failures.append("%s: frame 5 of trx_trace_ao_batch_dev differs in %d records" % (what, (batch[5].view(np.uint64) != want.view(np.uint64)).sum()))
            for f in (0, 7):
                other, other_i = _oracle_ao(case, prim, inst, sem, seed - 5 + f)
                if batch[f].tobytes() != other.tobytes() or (batch_i[f] != other_i).any():
                    failures.append("%s: frame %d of trx_trace_ao_batch_dev differs" % (what, f))
    print("closest-hit AO passes %s: %d targets as %s, sem 0 and 3" % (name, len(ND.CORE_TARGETS), "u2" if second else "u1"))
    assert not failures, "\n".join(failures)


# ---- d. sparse AO visibility -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [2, 3])
def test_sparse_visibility_draws_the_full_resolution_pixels_noise(trx, orc, cases, stride):
    """Under a u == 1.0 seed (as u1, as u2) and a theta == 0 seed of a represented pixel, the sparse pass's cells are the dense
    pass's bytes of their pixels - and the dense pass's bytes are the twin's."""
    case, _, _ = cases("cornell_64")
    w, h, n, sem = case.w, case.h, 4, 0
    with limit():
        d_prim, d_inst, prim, inst = case.primary(sem)
    wlo, hlo = lo_size(w, h, stride)
    for k, (tname, second) in enumerate((("last-1.0", False), ("first-1.0", True), ("0", True))):
        px, py, i = _surface_pixel(prim, w, 7 * k + stride)
        seed = ND.seed_for(px, py, ND.TARGETS[tname], second)
        _claimed(orc, px, py, seed, tname, second)
        frame0 = (seed - 1) & M32                                     # the target seed is sample 1 of 4
        phase = (py % stride) * stride + px % stride                  # the target pixel is its cell's pixel
        what = "stride %d phase %d %s as %s" % (stride, phase, tname, "u2" if second else "u1")
        with limit():
            dense = _visibility(case, d_prim, d_inst, n, case.radius, sem, (0, 1, 0), frame0=frame0)
        twin = visibility_counts(orc, case.osc, case.oview, w, h, prim, inst, sem, frame0, n, 0.01, case.radius)
        assert (dense == twin).all(), "%s: the dense pass differs from the twin in %d bytes" % (what, (dense != twin).sum())
        d_lo = _buf(wlo * hlo + 64, 0x5A)
        _sync()
        with limit():
            case.sc.trace_ao_visibility_sparse_dev(case.view, w, h, stride, phase, d_prim.data_ptr(), d_lo.data_ptr() + 32, n, case.radius, sem=sem,
                                                   frame0=frame0, ao_eps=0.01, d_primary_inst=d_inst.data_ptr())
            _torch().cuda.synchronize()
            case.sc.check()
        lo = d_lo.cpu().numpy()
        assert (lo[:32] == 0x5A).all() and (lo[32 + wlo * hlo:] == 0x5A).all(), what
        want = sparse_counts(dense, w, h, stride, phase)
        cell = (py // stride) * wlo + px // stride
        assert want[cell] == dense[i] != NO_SURFACE                   # the target pixel is represented
        bad = np.flatnonzero(lo[32:32 + wlo * hlo] != want)
        assert bad.size == 0, "%s: %d cells differ, first %s%s" % (what, bad.size, bad[:6], ", the target's among them" if cell in bad else "")


# ---- e. the rect light's sample --------------------------------------------------------------------------------------------------

def _search(prim, w, k, accept, what):
    """accept(px, py, i)'s first answer that is not None over the surface pixels from the k-th on."""
    for attempt in range(256):
        got = accept(*_surface_pixel(prim, w, k + attempt))
        if got is not None:
            return got
    raise AssertionError("no surface pixel " + what)


def _rect_frame0(orc, prim, w, k_light, sample, cast_of, j):
    """(what, frame0, target pixel index or None): j < 4: frame0 + 64 k_light + sample is the seed that gives a pixel the j-th
    edge target, the pixel one whose shadow ray the twin casts (cast_of(frame0) is the twin's cast mask) - an inert ray would
    hide the light point; j == 4: a frame0 whose sum wraps inside the samples."""
    if j == 4:
        return "frame0 + 64 k + f wraps at f = 2", (0x100000000 - 64 * k_light - 2) & M32, None
    tname, second = RECT_TARGETS[j]

    def accept(px, py, i):
        seed = ND.seed_for(px, py, ND.TARGETS[tname], second)
        frame0 = (seed - 64 * k_light - sample) & M32
        if not cast_of(frame0)[i]:
            return None
        _claimed(orc, px, py, seed, tname, second)
        return "%s as %s at pixel %d, %d" % (tname, "u2" if second else "u1", px, py), frame0, i
    return _search(prim, w, 5 * j + 1, accept, "whose shadow ray toward the rect light is cast")


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_rect_light_sample_at_the_rectangles_edges(trx, orc, cases, name):
    """Two lights, the rect one at k = 1, 4 samples, frame0 + 64 k + f the target seed at f = 2: trx_light_rays_dev and
    trx_trace_light_visibility_dev against the light twin.  The target pixel's ray is cast: its light point is in the output."""
    case, lc, _ = cases(name)
    w, h, n = case.w, case.h, case.w * case.h
    rect = LIGHTS[1]
    for sem in (0, 3):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem)
        geo = lc.geo(prim, inst)
        for j in range(5):
            what, frame0, i = _rect_frame0(orc, prim, w, 1, 2, lambda f0: LT.light_rays(orc, case.view, w, h, geo, rect, 1, f0, 2, EPS)[1], j)
            what = "%s sem %d %s (frame0 0x%08X)" % (name, sem, what, frame0)
            d_rays = _buf((n + 2) * 32, 0xA5)
            _sync()
            with limit():
                case.sc.light_rays_dev(case.view, w, h, rect.product(trx), d_prim.data_ptr(), d_rays.data_ptr() + 32, light_index=1, frame0=frame0,
                                       sample=2, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                _torch().cuda.synchronize()
                case.sc.check()
            got = d_rays.cpu().numpy().view(np.uint32).reshape(n + 2, 8)
            twin, cast = LT.light_rays(orc, case.view, w, h, geo, rect, 1, frame0, 2, EPS)
            want = np.full((n + 2, 8), SENTINEL, dtype=np.uint32)
            want[1:-1] = twin.view(np.uint32).reshape(-1, 8)
            diff = _differences(got[1:-1], want[1:-1], w, what + " trx_light_rays_dev")
            assert not diff and (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), diff
            assert cast.sum() > 30 and (i is None or (cast[i] and twin["tmax"][i] > 0)), what
            planes = lc.device_planes(d_prim, d_inst, LIGHTS, 4, sem, (0, 1, 0), frame0=frame0)
            expect = lc.expected(lc.planes(prim, inst, LIGHTS, frame0, 4, sem), (0, 1, 0))
            bad = np.flatnonzero(planes != expect)
            assert bad.size == 0, "%s trx_trace_light_visibility_dev: %d bytes differ, first %s" % (what, bad.size, bad[:6])
    print("rect light %s: %d edge targets (each at a pixel whose ray is cast) and a wrapping sum, rays and planes, sem 0 and 3" % (name, len(RECT_TARGETS)))


# ---- f. the bounce ---------------------------------------------------------------------------------------------------------------

def _two_chunks(trx, tiles, fn):
    """fn() under the default scratch cap and under one that holds one of the pass's two samples: two chunks."""
    lib = trx.load()
    try:
        fn("default cap")
        lib.trx_debug_ao_scratch_cap(BOUNCE_UNIT * tiles)
        fn("two chunks")
    finally:
        lib.trx_debug_ao_scratch_cap(0)


def _bounce_finds_a_surface(case, prim, inst, sem, seed, i):
    """On the oracle: pixel i's bounce ray under `seed` hits something."""
    rays = case.osc.ao_rays(case.oview, case.w, case.h, prim, inst, frame=seed & M32, ao_eps=EPS, threads=4)
    hits, _ = case.osc.trace_rays(rays, sem=sem, threads=4)
    return hits["prim"][i] != INVALID


def _bounce_target(orc, case, prim, inst, sem, tname, second, k):
    """(px, py, i, seed): a surface pixel given the target as the u1 / u2 of its bounce ray under `seed`, the ray one that
    finds a surface - so that the direction reaches a secondary hit and what is computed there."""
    def accept(px, py, i):
        seed = ND.seed_for(px, py, ND.TARGETS[tname], second)
        if not _bounce_finds_a_surface(case, prim, inst, sem, seed, i):
            return None
        _claimed(orc, px, py, seed, tname, second)
        return px, py, i, seed
    return _search(prim, case.w, k, accept, "whose bounce ray finds a surface")


def _indirect_frame0s(orc, case, gi, prim, inst, sem, second):
    """(what, frame0, target pixel index or None) of two-sample passes: the bounce ray's seed at sample 1 is a core target (as
    u1 / u2 by `second`) at a pixel whose bounce finds a surface; the rect light's sample at a secondary hit (seed frame0 + 64
    + 1) is an edge target, at a pixel whose bounce finds a surface from which the twin casts the shadow ray toward the rect
    light; and a frame0 whose sums wrap."""
    w, h = case.w, case.h
    out = []
    for k, tname in enumerate(ND.CORE_TARGETS):
        px, py, i, seed = _bounce_target(orc, case, prim, inst, sem, tname, second, 3 * k + second)
        out.append(("bounce %s as %s at pixel %d, %d" % (tname, "u2" if second else "u1", px, py), (seed - 1) & M32, i))
    for k, (tname, sec) in enumerate(RECT_TARGETS):
        if sec != second:
            continue

        def accept(px, py, i):
            seed = ND.seed_for(px, py, ND.TARGETS[tname], sec)
            frame0 = (seed - 64 - 1) & M32
            if not _bounce_finds_a_surface(case, prim, inst, sem, frame0 + 1, i):
                return None
            key = (frame0 + 1, float(EPS), sem, hash(prim.tobytes()), hash(np.asarray(inst).tobytes()))     # (IT.indirect's cache key)
            if key not in gi.cache:
                gi.cache[key] = IT.bounce(orc, case.osc, case.oview, w, h, prim, inst, gi.recs, gi.w2o, frame0 + 1, EPS, sem)
            b_rays, b_hits, _, b_attr = gi.cache[key]
            _, cast = IT.secondary_rays(orc, w, h, b_rays, b_hits, b_attr, LIGHTS[1], 1, frame0, 1, EPS)
            if not cast[i]:
                return None
            _claimed(orc, px, py, seed, tname, sec)
            return "secondary light sample %s as %s at pixel %d, %d" % (tname, "u2" if sec else "u1", px, py), frame0, i
        out.append(_search(prim, w, 11 * k, accept, "whose secondary hit casts a shadow ray toward the rect light"))
    out.append(("wrapping frame0", 0xFFFFFFFF, None))
    return out


@pytest.mark.parametrize("second", [False, True], ids=["u1", "u2"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_indirect_dense_and_sparse_at_the_targets(trx, orc, cases, name, second):
    """trx_trace_indirect_dev and trx_trace_indirect_sparse_dev (stride 2, the phase that makes the target pixel its cell's
    pixel) against the indirect twin, two lights (the rect one at k = 1), two samples, under the default scratch cap and in
    two chunks."""
    case, _, gi = cases(name)
    w, h, sem = case.w, case.h, 3 if second else 0
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    wlo, hlo = lo_size(w, h, 2)
    lo_tiles = ((wlo + 7) // 8) * ((hlo + 7) // 8)
    with limit():
        d_prim, d_inst, prim, inst = case.primary(sem)
    runs = _indirect_frame0s(orc, case, gi, prim, inst, sem, second)
    surf = LT.surface(prim)
    failures = []

    def dense(cap):
        for what, frame0, _ in runs:
            got, before = gi.device(d_prim, d_inst, LIGHTS, 2, sem, (0, 1, 0), frame0=frame0)
            want = gi.expected(gi.twin(prim, inst, LIGHTS, frame0, 2, sem), before, (0, 1, 0))
            if (got != want).any():
                failures.append("%s sem %d %s, %s: trx_trace_indirect_dev differs in %d bytes" % (name, sem, what, cap, (got != want).sum()))

    def sparse(cap):
        for what, frame0, i in runs:
            px, py = (i % w, i // w) if i is not None else (1, 1)
            phase = (py % 2) * 2 + px % 2                          # the target pixel is its cell's pixel
            d_lo = _buf((wlo * hlo + 16) * 4, 0x5A)
            _sync()
            with limit():
                case.sc.trace_indirect_sparse_dev(case.view, w, h, 2, phase, [l.product(trx) for l in LIGHTS], d_prim.data_ptr(),
                                                  d_lo.data_ptr() + 32, n_samples=2, sem=sem, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS,
                                                  bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr())
                _torch().cuda.synchronize()
                case.sc.check()
            lo = d_lo.cpu().numpy()
            assert (lo[:32] == 0x5A).all() and (lo[32 + wlo * hlo * 4:] == 0x5A).all(), what
            values = gi.twin(prim, inst, LIGHTS, frame0, 2, sem)
            want = IST.sparse_values(values, prim, w, h, 2, phase)
            if i is not None:      # the target's cell stands for the target pixel, a surface: it holds the dense pass's value there
                cell = (py // 2) * wlo + px // 2
                assert surf[i] and want[cell].tobytes() == values[i].tobytes(), what
            got = lo[32:32 + wlo * hlo * 4].view(np.uint32)
            if (got != want.view(np.uint32)).any():
                failures.append("%s sem %d %s, %s: trx_trace_indirect_sparse_dev phase %d differs in %d cells" % (
                    name, sem, what, cap, phase, (got != want.view(np.uint32)).sum()))

    _two_chunks(trx, tiles, dense)
    _two_chunks(trx, lo_tiles, sparse)
    values = gi.twin(prim, inst, LIGHTS, runs[0][1], 2, sem)
    assert (values[surf] > 0).mean() > 0.05                                  # (not vacuous)
    print("indirect %s sem %d: %d frame0s (core targets as %s at pixels whose bounce hits, edge targets of the secondary light sample at pixels "
          "whose shadow ray is cast, a wrap), dense and stride 2 with the target's phase, two caps" % (name, sem, len(runs), "u2" if second else "u1"))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_secondary_shadow_rays_at_the_rectangles_edges(trx, orc, cases, name):
    """trx_bounce_light_rays_dev: bounce rays under every core target as u1 and as u2, at a pixel whose bounce finds a surface
    (the device's own rays, hits and attribute records, which the tests above and tests/test_gpu_indirect.py hold to the
    twin); the rect light's sample at an edge target - at a pixel whose secondary shadow ray the twin casts - or under a
    wrapping sum, the five taken in turn."""
    case, _, _ = cases(name)
    w, h, n, sem = case.w, case.h, case.w * case.h, 0
    rect = LIGHTS[1]
    with limit():
        d_prim, d_inst, prim, inst = case.primary(sem)
    for k, tname in enumerate(ND.CORE_TARGETS):
        for second in (False, True):
            _, _, at, bounce_seed = _bounce_target(orc, case, prim, inst, sem, tname, second, 13 * k + 2 + second)
            (d_br, d_bh, _, d_ba), (b_rays, b_hits, b_attr) = _device_bounce(case, d_prim, d_inst, (0, 1, 0), bounce_seed, sem)
            has = IT.bounce_surface(b_rays, b_hits)
            assert has.sum() > 10 and has[at], (tname, second)
            what, frame0, i = _rect_frame0(orc, prim, w, 1, 2, lambda f0: IT.secondary_rays(orc, w, h, b_rays, b_hits, b_attr, rect, 1, f0, 2, EPS)[1],
                                           (2 * k + second) % 5)
            d_rays = _buf((n + 2) * 32, 0xA5)
            _sync()
            with limit():
                case.sc.bounce_light_rays_dev(w, h, rect.product(trx), d_br.data_ptr(), d_bh.data_ptr(), d_ba.data_ptr(), d_rays.data_ptr() + 32,
                                              light_index=1, frame0=frame0, sample=2, shadow_eps=EPS)
                _torch().cuda.synchronize()
                case.sc.check()
            got = d_rays.cpu().numpy().view(np.uint32).reshape(n + 2, 8)
            twin, cast = IT.secondary_rays(orc, w, h, b_rays, b_hits, b_attr, rect, 1, frame0, 2, EPS)
            what = "%s bounce %s as %s, light sample %s" % (name, tname, "u2" if second else "u1", what)
            diff = _differences(got[1:-1], twin.view(np.uint32).reshape(-1, 8), w, what)
            assert not diff and (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), diff
            assert cast.sum() > 5 and (i is None or (has[i] and cast[i] and twin["tmax"][i] > 0)), what


# ---- g. the dense leg --------------------------------------------------------------------------------------------------------------

def test_dense_leg_half_a_million_rays(trx, orc, dom):
    """256 x 256 hand-made records on the single-level scene under the eight committed seeds: all 2^19 rays of trx_ao_rays_dev
    equal orc_ao_rays'.  tests/test_noise_domain.py asserts what the seeds reach: the small-angle branch, every quadrant word,
    theta == fl(2 pi) and u1 == 1.0."""
    w = h = ND.DENSE
    oview = orc.view_from_bytes(bytes(dom.dense_view))
    rec, inst, d_prim, d_inst = dom.records("single", w, h)
    failures, n_small, n_quadrant = [], 0, np.zeros(5, dtype=np.int64)
    for seed in ND.DENSE_SEEDS:
        got = dom.device_rays("single", dom.dense_view, w, h, d_prim, d_inst, seed, INF, 0.01)
        want = dom.oracle_rays("single", oview, w, h, rec, inst, seed, INF, 0.01, threads=8)
        _, small, n = ND.classify_image(ND.image_hashes(w, h, seed, second=True))
        n_small += int(small.sum())
        n_quadrant += np.bincount(n, minlength=5)
        bad = np.flatnonzero((got != want).any(1))
        if bad.size:
            failures.append(_differences(got, want, w, "seed 0x%08X" % seed) + "; of them %d in the small-angle branch, by quadrant word %s" % (
                small[bad].sum(), np.bincount(n[bad], minlength=5)))
    (p1, _), (p2, _) = ND.DENSE_U1_ONE, ND.DENSE_U2_ONE
    assert _noise(orc, *p1, ND.DENSE_SEEDS[6], False) == 1.0 and _noise(orc, *p2, ND.DENSE_SEEDS[7], True) == 1.0
    print("dense leg: %d rays, %d in the small-angle branch, by quadrant word %s" % (len(ND.DENSE_SEEDS) * w * h, n_small, n_quadrant))
    assert not failures, "\n".join(failures)
