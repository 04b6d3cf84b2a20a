"""AO visibility on the GPU, byte for byte: trx_ao_rays_dev writes the twin's rays (tests/ao_visibility_twin.py) and the
inert ray, trx_trace_ao_visibility_dev the twin's counts - fed the device's own primary records, which test_gpu_parity.py and
test_gpu_instances.py hold to the oracle - on single-level, two-level and transformed scenes, in both layouts, for 1, 8 and
64 samples, a finite radius and +inf, every semantics word, and with a scratch cap small enough that the chunk loops run.
No record is left out of any comparison.

cornell_64_pipe and soup_52x44_pipe are the padded twins of those goldens (helpers.padded_flat): the pass's any-hit rays
launch takes the pipelined walk on them.  A twin shares its base case's Python twin answers, and every count it produces is
also compared byte for byte with what the unpadded scene gives for the same arguments."""
import ctypes as C

import numpy as np
import pytest

from ao_visibility_twin import (THREADS, GOLDEN_RADIUS, INSTANCED_RADIUS, INVALID, NO_SURFACE, ao_rays, golden_case, instanced_case,
                                record_map, stored_tmax, visibility_counts)
from helpers import ALL_SEMS, assert_walk_kinds, padded_flat

pytestmark = pytest.mark.gpu
INF = float("inf")
UNIT = 64 * 32 + 64   # scratch bytes per tile and sample: 64 rays and their flags


def _torch():
    import torch
    return torch


class Case:
    """A scene on the device and on the oracle, with the device's primary records per (semantics, shard, stream)."""

    def __init__(self, trx, orc, name):
        self.trx, self.orc, self.name = trx, orc, name
        if name == "instanced":
            flat, self.view, _, _, self.w, self.h = instanced_case(trx, orc)
            self.sc = trx.Scene(flat)
            # the oracle walks with the world-to-object rows the kernels use
            _, _, self.osc, self.oview, _, _ = instanced_case(trx, orc, w2o=self.sc.instance_world_to_object())
            self.radius = INSTANCED_RADIUS
        else:
            from tray_racing_amd import _lib
            self.osc, self.oview, self.w, self.h, g = golden_case(trx, orc, name)
            n = g["tri_verts"].shape[0]
            self.flat = trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n), [0, n])
            self.sc = trx.Scene(self.flat)
            self.view = _lib.View()
            C.memmove(C.byref(self.view), g["view"].tobytes(), C.sizeof(self.view))
            self.radius = GOLDEN_RADIUS.get(name, 1.0)
        self.transformed = name == "instanced"
        self.base = None          # (a padded twin: the case of the unpadded scene)
        self._rays, self._unoccluded = {}, {}

    def close(self):
        self.sc.close()

    def primary(self, sem, shard=(0, 1, 0), stream=0):
        """(d_prim, d_inst tensors laid out by `shard`, the records in pixel order, the instance ids in pixel order)."""
        torch = _torch()
        from tray_racing_amd import _lib as L
        pix, rec, n = record_map(self.w, self.h, shard)
        d_prim = torch.full((n * 8,), 0xEE, dtype=torch.uint8, device="cuda")
        d_inst = torch.full((n * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        L.check(self.sc._lib.trx_trace_primary_inst_dev(self.sc.handle, C.byref(self.view), self.w, self.h, L.Shard(*shard, 0), sem,
                                                        C.c_void_p(d_prim.data_ptr()), C.c_void_p(d_inst.data_ptr()),
                                                        C.c_void_p(stream)))
        torch.cuda.synchronize()
        prim = np.zeros(self.w * self.h, dtype=self.orc.HIT_DTYPE)
        prim["t"], prim["prim"] = np.inf, INVALID          # pixels of other shards: no surface for the twin
        inst = np.full(self.w * self.h, INVALID, dtype=np.uint32)
        prim[pix] = d_prim.cpu().numpy().view(self.orc.HIT_DTYPE)[rec]
        inst[pix] = d_inst.cpu().numpy().view(np.uint32)[rec]
        return d_prim, d_inst, prim, inst

    def unoccluded(self, sem, prim, inst, frame0, n_samples, radius, eps=0.01):
        """[n_samples, w * h] bool: the twin's answer per seed (rays are built once per seed and reused across radii)."""
        whole = (sem, frame0, n_samples, radius, eps, hash(prim.tobytes()), hash(inst.tobytes()))
        if whole in self._unoccluded:      # (asked before, by this case or by its padded twin)
            return self._unoccluded[whole]
        out = np.zeros((n_samples, self.w * self.h), dtype=bool)
        for f in range(n_samples):
            key = (frame0 + f, eps, hash(prim.tobytes()), hash(inst.tobytes()))
            if key not in self._rays:
                self._rays[key] = ao_rays(self.orc, self.osc, self.oview, self.w, self.h, prim, inst, frame0 + f, eps, INF)
            rays, surface = self._rays[key]
            rays = rays.copy()
            rays["tmax"][surface] = stored_tmax(radius)
            hits, _ = self.osc.trace_rays(rays, sem=sem, threads=THREADS)
            assert (hits["prim"][~surface] == INVALID).all()
            out[f] = hits["prim"] == INVALID
        self._unoccluded[whole] = (out, surface)
        return out, surface


class PaddedCase(Case):
    """The padded twin of a single-level golden case: the base case's oracle scene, views and cached twin answers (the very
    dictionaries), and a padded scene on the device whose explicit-ray launches take the pipelined walk."""

    def __init__(self, base):
        self.__dict__.update(base.__dict__)
        self.base, self.name = base, base.name + "_pipe"
        self.sc = self.trx.Scene(padded_flat(self.trx, base.flat))
        self.assert_walks()

    def assert_walks(self):
        """Asked again by every test that takes the twin (make_case)."""
        for mode in (self.trx.MODE_RAYS, self.trx.MODE_AO):
            assert_walk_kinds(self.trx, self.base.sc, self.sc, mode)


def make_case(trx, orc, made, name):
    """The case `name` of a module's `made` dictionary; a name ending in _pipe is the padded twin of the case before it."""
    if name not in made:
        made[name] = PaddedCase(make_case(trx, orc, made, name[:-len("_pipe")])) if name.endswith("_pipe") else Case(trx, orc, name)
    if made[name].base is not None:
        made[name].assert_walks()
    return made[name]


def _expected_counts(unocc, surface, n, shard, w, h, fill):
    """The output buffer the device must produce: `fill` everywhere, the counts of the first n seeds at the shard's records."""
    pix, rec, size = record_map(w, h, shard)
    want = np.full(size, fill, dtype=np.uint8)
    counts = np.where(surface, unocc[:n].sum(0), NO_SURFACE).astype(np.uint8)
    want[rec] = counts[pix]
    return want


def _visibility(case, d_prim, d_inst, n, radius, sem, shard, frame0=0, stream=0, fill=0x5A, eps=0.01):
    """The pass's output buffer; on a padded twin also checked, byte for byte, against the unpadded scene's."""
    torch = _torch()
    _, _, size = record_map(case.w, case.h, shard)
    outs = []
    for sc in (case.sc,) if case.base is None else (case.sc, case.base.sc):
        d_out = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_out.data_ptr(), n, radius, sem=sem,
                                   frame0=frame0, ao_eps=eps, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0,
                                   shard=(*shard, 0), stream=stream)
        torch.cuda.synchronize()
        sc.check()
        outs.append(d_out.cpu().numpy())
    assert len(outs) == 1 or (outs[0] == outs[1]).all(), "%s: %d bytes differ from the unpadded scene's" % (case.name, (outs[0] != outs[1]).sum())
    return outs[0]


@pytest.fixture(scope="module")
def cases(trx, orc):
    made = {}

    def get(name):
        return make_case(trx, orc, made, name)
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


# ---- trx_ao_rays_dev ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shard,radius,own_stream", [
    ("cornell_64", (0, 1, 0), 1.4, False), ("cornell_64", (0, 1, 1), INF, True),
    ("soup_52x44", (1, 3, 0), 0.8, False), ("soup_52x44", (1, 3, 1), 0.8, True), ("soup_52x44", (0, 1, 1), INF, False),
    ("cornell_tlas_48", (1, 3, 1), 1.4, False), ("cornell_tlas_48", (0, 1, 0), INF, True),
    ("instanced", (0, 1, 0), 1.6, True), ("instanced", (1, 3, 1), INF, False), ("instanced", (1, 3, 0), 1.6, False)])
def test_ao_rays_are_the_twins_rays_and_the_inert_ray(trx, orc, cases, name, shard, radius, own_stream):
    torch = _torch()
    case = cases(name)
    st = torch.cuda.Stream() if own_stream else None
    stream = st.cuda_stream if st else 0
    for sem, frame, eps in ((0, 0, 0.01), (3, 9, 0.0001)):
        d_prim, d_inst, prim, inst = case.primary(sem, shard, stream)
        pix, rec, size = record_map(case.w, case.h, shard)
        d_rays = torch.full((size * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        case.sc.ao_rays_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_rays.data_ptr(), radius, frame=frame, ao_eps=eps,
                            d_primary_inst=d_inst.data_ptr(), shard=(*shard, 0), stream=stream)
        torch.cuda.synchronize()
        got = d_rays.cpu().numpy().view(np.uint32).reshape(size, 8)
        twin, surface = ao_rays(orc, case.osc, case.oview, case.w, case.h, prim, inst, frame, eps, radius)
        want = np.full((size, 8), 0xA5A5A5A5, dtype=np.uint32)       # records outside the shard or the image: the sentinel
        want[rec] = twin.view(np.uint32).reshape(-1, 8)[pix]
        what = "%s shard %s radius %g sem %d" % (name, shard, radius, sem)
        assert surface[pix].sum() > 30 and (~surface[pix]).sum() > 30, what
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, "%s: %d of %d records differ, first %s: %s != %s" % (what, bad.size, size, bad[:4], got[bad[:1]], want[bad[:1]])
        inert = np.array([0, 0, 0, 0, 0, 0, 0, 0xBF800000], dtype=np.uint32)
        assert (got[rec[~surface[pix]]] == inert).all(), what
        if (shard[1] > 1 and shard[2] == 0) or ((case.w % 8 or case.h % 8) and shard[2] == 1):
            assert (want == 0xA5A5A5A5).all(1).any(), what           # (some record really is outside)


def test_ao_rays_and_visibility_need_instance_ids_on_transformed_scenes(trx, cases):
    torch = _torch()
    case = cases("instanced")
    d_prim, d_inst, _, _ = case.primary(0)
    n = case.w * case.h
    d_rays = torch.full((n * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(trx.TrxError, match="instance transforms") as e:
        case.sc.ao_rays_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_rays.data_ptr(), 1.0)
    assert e.value.code == -1
    with pytest.raises(trx.TrxError, match="instance transforms"):
        case.sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_out.data_ptr(), 4, 1.0)
    for bad in (0.0, -1.0, float("nan"), -INF):
        with pytest.raises(trx.TrxError, match="ao_radius"):
            case.sc.ao_rays_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_rays.data_ptr(), bad, d_primary_inst=d_inst.data_ptr())
    torch.cuda.synchronize()
    assert (d_rays.cpu().numpy() == 0xA5).all() and (d_out.cpu().numpy() == 0x5A).all()


# ---- trx_trace_ao_visibility_dev --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48", "instanced", "cornell_64_pipe"])
def test_visibility_counts_equal_the_twin(trx, orc, cases, name):
    """Single-level, two-level and transformed scenes; image and shard layouts, shard (1, 3) among them; 1, 8 and 64 samples;
    the finite radius of tests/test_ao_visibility.py and +inf; every semantics word (64 samples under TRX_SEM_HLSL and
    TRX_SEM_CPU, 1 and 8 under all eight); a non-null stream."""
    torch = _torch()
    case = cases(name)
    st = torch.cuda.Stream()
    for sem in ALL_SEMS:
        ns = (1, 8, 64) if sem in (0, 3) else (1, 8)
        for shard, stream in (((0, 1, 0), 0), ((1, 3, 1), st.cuda_stream)) if sem in (0, 3, 5) else (((0, 1, 1), 0),):
            d_prim, d_inst, prim, inst = case.primary(sem, shard, stream)
            for radius in (case.radius, INF):
                unocc, surface = case.unoccluded(sem, prim, inst, 3, max(ns), radius)
                for n in ns:
                    got = _visibility(case, d_prim, d_inst, n, radius, sem, shard, frame0=3, stream=stream)
                    want = _expected_counts(unocc, surface, n, shard, case.w, case.h, 0x5A)
                    bad = np.flatnonzero(got != want)
                    assert bad.size == 0, "%s sem %d shard %s radius %g n %d: %d of %d bytes differ, first %s: %s != %s" % (
                        name, sem, shard, radius, n, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])
                if shard[1] == 1 and radius != INF and sem in (0, 3):
                    c8 = want if ns[-1] == 8 else _expected_counts(unocc, surface, 8, shard, case.w, case.h, 0x5A)
                    surf = c8[c8 != NO_SURFACE]
                    assert ((surf > 0) & (surf < 8)).mean() >= 0.05 and (surf == 0).any() and (surf == 8).any()


@pytest.mark.parametrize("name", ["cornell_64", "instanced", "cornell_64_pipe"])
def test_chunk_loops_give_the_same_counts(trx, orc, cases, name):
    """A scratch cap below the pass's need: samples in several chunks (counts added to), tiles in several chunks, both."""
    lib = trx.load()
    case = cases(name)
    tiles = ((case.w + 7) // 8) * ((case.h + 7) // 8)
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (0, 1, 1))):
            d_prim, d_inst, prim, inst = case.primary(sem, shard)
            unocc, surface = case.unoccluded(sem, prim, inst, 0, 8, case.radius)
            want = _expected_counts(unocc, surface, 8, shard, case.w, case.h, 0x5A)
            for cap in (UNIT * tiles * 3, UNIT * tiles, UNIT * 10, UNIT * (tiles // 2 + 1) * 2, 1):
                lib.trx_debug_ao_scratch_cap(cap)
                got = _visibility(case, d_prim, d_inst, 8, case.radius, sem, shard)
                assert (got == want).all(), "%s sem %d cap %d: %d bytes differ" % (name, sem, cap, (got != want).sum())
    finally:
        lib.trx_debug_ao_scratch_cap(0)


@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "cornell_tlas_48", "instanced", "cornell_64_pipe", "soup_52x44_pipe"])
def test_infinite_radius_counts_are_the_misses_of_the_ao_batch(trx, cases, name):
    torch = _torch()
    case = cases(name)
    n_px = case.w * case.h
    for sem in (0, 3, 6):
        d_prim, d_inst, prim, _ = case.primary(sem)
        surface = (prim["t"] < 3.4028234663852886e38) & (prim["prim"] != INVALID)
        for n, frame0 in ((8, 0), (3, 11)):
            d_ao = torch.zeros((n * n_px * 8,), dtype=torch.uint8, device="cuda")
            case.sc.trace_ao_batch_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_ao.data_ptr(), n_px, n, sem=sem, frame0=frame0,
                                       d_primary_inst=d_inst.data_ptr())
            torch.cuda.synchronize()
            ao = d_ao.cpu().numpy().view(trx.HIT_DTYPE).reshape(n, n_px)
            hits = (ao["prim"] != INVALID).sum(0)
            got = _visibility(case, d_prim, d_inst, n, INF, sem, (0, 1, 0), frame0=frame0)
            assert (got[~surface] == NO_SURFACE).all() and (got[surface] == n - hits[surface]).all(), (name, sem, n)
            assert 0 < hits[surface].sum() < n * surface.sum()


def test_refusals_leave_the_output_untouched(trx, cases):
    torch = _torch()
    case = cases("cornell_64")
    d_prim, d_inst, _, _ = case.primary(0)
    d_out = torch.full((case.w * case.h,), 0x5A, dtype=torch.uint8, device="cuda")

    def call(n, radius, sem=0):
        case.sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_out.data_ptr(), n, radius, sem=sem)

    for n in (0, 65):
        with pytest.raises(trx.TrxError, match="n_samples") as e:
            call(n, 1.0)
        assert e.value.code == -1
        with pytest.raises(trx.TrxError, match="n_samples"):
            case.sc.trace_ao_visibility(case.view, case.w, case.h, n, 1.0)
    for radius in (0.0, -2.0, float("nan")):
        with pytest.raises(trx.TrxError, match="ao_radius") as e:
            call(4, radius)
        assert e.value.code == -1
        with pytest.raises(trx.TrxError, match="ao_radius"):
            case.sc.trace_ao_visibility(case.view, case.w, case.h, 4, radius)
    with pytest.raises(trx.TrxError, match="semantics"):
        call(4, 1.0, sem=8)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    call(4, 1.0)   # and the scene is still usable
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() != 0x5A).any()


def test_host_buffer_form_equals_the_twin(trx, orc, cases):
    for name in ("cornell_tlas_48", "instanced"):
        case = cases(name)
        for sem in (0, 3):
            _, _, prim, inst = case.primary(sem)
            got, ms = case.sc.trace_ao_visibility(case.view, case.w, case.h, 8, case.radius, sem=sem, frame0=2)
            want = visibility_counts(orc, case.osc, case.oview, case.w, case.h, prim, inst, sem, 2, 8, 0.01, case.radius)
            assert ms > 0 and (got == want).all(), (name, sem)


def test_device_bytes_count_the_scratch_once(trx, orc):
    torch = _torch()
    case = Case(trx, orc, "cornell_64")
    try:
        d_prim, d_inst, _, _ = case.primary(0)
        n, tiles = 4, ((case.w + 7) // 8) * ((case.h + 7) // 8)
        # the rays launch of this size first, on the same stream: the launch slot's stack spill area is then sized for it
        d_rays = torch.zeros((tiles * n * 64 * 32,), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((tiles * n * 64,), dtype=torch.uint8, device="cuda")
        case.sc.trace_occluded_dev(d_rays.data_ptr(), tiles * n * 64, d_flags.data_ptr())
        torch.cuda.synchronize()
        before = case.sc.device_bytes
        _visibility(case, d_prim, d_inst, n, 1.4, 0, (0, 1, 0))
        first = case.sc.device_bytes
        assert first - before == tiles * n * UNIT
        _visibility(case, d_prim, d_inst, n, INF, 3, (0, 1, 0))
        _visibility(case, d_prim, d_inst, 2, 1.4, 0, (1, 3, 1))
        assert case.sc.device_bytes == first
    finally:
        case.close()


def test_cli_png_shades_with_the_visibility_counts(trx, orc, tmp_path):
    """--png with --ao-samples / --ao-radius: the AO term is count / N (0 where there is no surface), gamma 2.2 to u8."""
    import os
    import struct
    import subprocess
    import zlib
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "tray_racing_hip")
    w, h, n, radius = 96, 64, 4, 1.4
    r = subprocess.run([cli, "-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1",
                        "--png", "--cpu-semantics", "--ao-samples", str(n), "--ao-radius", str(radius)], capture_output=True,
                       text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    data = (tmp_path / "cornell_rend.png").read_bytes()
    pos, idat = 8, b""
    while pos < len(data):
        size, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + size]
        pos += 12 + size
    img = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)[:, 1:].reshape(h, w, 4)
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    ov = orc.view_from_bytes(trx.view_from_camera(eye, look, fov, w, h))
    osc = orc.Scene.from_flat(flat)
    prim, inst, _ = osc.trace_primary_inst(ov, w, h, sem=3)
    counts = visibility_counts(orc, osc, ov, w, h, prim, inst, 3, 0, n, 0.0001, radius)
    # (count / 4 to the power 2.2 times 255 is 0, 12.07, 55.5, 135.4 or 255: no value near an integer, so exact)
    col = np.where(counts == NO_SURFACE, 0.0, counts / float(n))
    want = (np.power(col, 2.2) * 255.0).astype(np.uint8).reshape(h, w)
    assert (img[..., 3] == 255).all() and (img[..., 0] == want).all() and (img[..., 1] == want).all() and (img[..., 2] == want).all()
    assert len(np.unique(want)) >= 4
    # without the flags the image is the reference's shading (tests/test_cli.py), another image
    r = subprocess.run([cli, "-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1",
                        "--png", "--cpu-semantics"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and (tmp_path / "cornell_rend.png").read_bytes() != data
