"""Caller records on the GPU (include/trx.h, "CALLER RECORDS"): every *_dev pass that indexes the scene's tables with a primary
record of the caller's, fed records the library did not write - ids at, just past and far past the tables' ends, t on both
sides of FLT_MAX (tests/caller_records.py) - and the suite's own sentinel frame.  Whole output buffers, sentinels included,
against the oracle or the twin over the same records, bit for bit; and every undoctored pixel against the same pass over
the clean records, so a doctored neighbour cannot disturb a wave unseen.

ORDER.  The tests of the ids just past the tables (n_tris, n_tris + 1, n_instances, n_instances + 1) come first: run with
-x, a read the rule does not bound shows there as a wrong value and stops the run before an id far outside is handed to it.

Every step that runs on the GPU sits under a time limit of its own (test_gpu_light.limit)."""
import ctypes as C

import numpy as np
import pytest

import indirect_sparse_twin as IST
import indirect_twin as IT
import light_twin as LT
from ao_sparse_twin import ao_upsample, cell_pixels, lo_size, sparse_counts
from ao_visibility_twin import NO_SURFACE, ao_rays, record_map, surface_records, visibility_counts
from caller_records import INVALID, TILE, doctor, entries, pick_pixels
from heat_twin import COST_DTYPE
from hit_attr_twin import tri_records
from image_twin import TERM_DTYPE
from test_gpu_ao_visibility import UNIT, make_case
from test_gpu_indirect import UNIT as GI_UNIT
from test_gpu_light import FILL, INERT, _buf, _dev, _mixed, limit

pytestmark = pytest.mark.gpu
CASES = ["cornell_64", "soup_52x44", "soup_52x44_pipe", "cornell_tlas_48", "instanced"]
# soup_52x44_pipe is the padded twin: n_tris is the padded extent, the AO pass and every rays launch take the pipelined walk.
# Its appended records are zero-area triangles, so a surface record that names one (the table's n_tris - 1) has the normal
# 0/0: the AO ray writer's direction is three NaNs, whose sign and payload are the platform's - those words alone are
# compared as "NaN on both sides" (_nan_words); everything downstream of them (inert shadow rays, counts, values) has none.
EPS, SEM, FRAME, ALBEDO, SLACK = 0.01, 3, 5, 0.6, 37
FILL32 = 0x5A5A5A5A
f32 = np.float32


def _torch():
    import torch
    return torch


def _sync():
    with limit():
        _torch().cuda.synchronize()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


def _nan_words(got, want, rows, what):
    """The direction words (4..6) of the ray records `rows`: NaN in `got` and in `want` alike - asserted - and then made one
    pattern in copies of both, so that the byte comparison that follows holds every other word of every record."""
    got, want = got.copy(), want.copy()
    g, w = got[rows, 4:7].view(np.float32), want[rows, 4:7].view(np.float32)
    assert np.isnan(g).all() and np.isnan(w).all(), "%s: %d / %d of %d direction words are NaN" % (what, np.isnan(g).sum(), np.isnan(w).sum(), g.size)
    got[rows, 4:7] = want[rows, 4:7] = 0x7FC00000
    return got, want


class Doctored:
    """A case of tests/test_gpu_ao_visibility.py, the device's own primary frame of it (with instance ids) and a copy doctored
    with the table: one whole 8x8 tile (miss entries only: a wave has nothing usable), single pixels scattered over other tiles, the first and the last pixel of the image,
    and a pixel of a ragged edge tile where the size has one."""

    def __init__(self, trx, orc, case, near):
        self.trx, self.orc, self.case, self.w, self.h = trx, orc, case, case.w, case.h
        self.n = self.w * self.h
        flat = case.sc.flat
        self.n_tris, self.n_inst = int(flat.n_tris), int(np.asarray(flat.instance_offsets).size)
        self.osc = case.osc
        if case.base is not None:
            # a padded twin: the device's extent is the padded one, and so must the oracle's be (the base case's scene ends earlier)
            assert self.n_tris > case.osc.tris.shape[0] and case.sc.walk_kind(trx.MODE_AO) == trx.WALK_PIPELINED
            self.osc = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start)
        assert int(self.osc.c.n_tris) == self.n_tris and int(self.osc.c.n_instances) == self.n_inst
        self.tlas = self.n_inst > 0
        self.recs = tri_records(self.osc.verts)
        self.w2o = self.osc.w2o if case.transformed else None
        with limit():
            self.d_prim, self.d_inst, self.prim, self.inst = case.primary(SEM)
        table = entries(self.n_tris, self.n_inst, near=near)
        surf = surface_records(self.prim, self.n_tris)
        self.pixels, self.tile = pick_pixels(self.w, self.h, len(table), surf)
        self.dp, self.di, _, _, self.is_surface = doctor(self.prim, self.inst, self.pixels, table)
        self.miss_px = self.pixels[~self.is_surface]
        self.clean = np.ones(self.n, dtype=bool)
        self.clean[self.pixels] = False
        assert (self.clean & surf).sum() >= 200, "%s: %d undoctored surface pixels" % (case.name, (self.clean & surf).sum())
        assert self.tile.size == TILE and (self.pixels[:TILE] == self.tile).all() and 0 in self.pixels and self.n - 1 in self.pixels
        # the whole tile: not one surface record left for a wave, where most of its pixels were surface pixels
        assert not self.is_surface[:TILE].any() and not surface_records(self.dp, self.n_tris)[self.tile].any()
        assert surf[self.tile].sum() >= 32, "%s: the doctored tile had %d surface pixels" % (case.name, surf[self.tile].sum())
        assert len(self.pixels) - TILE >= len(table)
        assert not (self.w % 8 or self.h % 8) or ((self.pixels % self.w) // 8 == self.w // 8).any() or ((self.pixels // self.w) // 8 == self.h // 8).any()
        # doctored pixels on and off each sparse phase's grid
        for phase in (0, 3):
            on = (self.pixels % self.w % 2 == phase % 2) & (self.pixels // self.w % 2 == phase // 2)
            assert on.any() and (~on).any()
        self.d_dp, self.d_di = _dev(self.dp), _dev(self.di)
        self._twin = {}

    def twin(self, key, make):
        if key not in self._twin:
            self._twin[key] = make()
        return self._twin[key]

    def both(self, run):
        """run(d_prim, d_inst) over the doctored and over the clean records; the undoctored records of the two must agree."""
        got = run(self.d_dp, self.d_di)
        clean = run(self.d_prim, self.d_inst)
        return got, clean

    def finish(self):
        with limit():
            _torch().cuda.synchronize()
            self.case.sc.check()


@pytest.fixture(scope="module")
def cases(trx, orc):
    made, docs = {}, {}

    def get(name, near):
        case = make_case(trx, orc, made, name)
        if (name, near) not in docs:
            docs[name, near] = Doctored(trx, orc, case, near)
        return docs[name, near]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


# ---- site 1: the AO pass's refill (trx_trace_ao_dev, _ao_inst_dev, _ao_batch_dev, _ao_masked_dev, trx_count_ao, trx_count_ao_per_ray)

def _ao_passes(dc):
    torch = _torch()
    from tray_racing_amd import _lib as L
    case, sc, n, w, h = dc.case, dc.case.sc, dc.n, dc.w, dc.h
    ids = dc.di if dc.tlas else np.full(n, INVALID, dtype=np.uint32)
    want = [dc.osc.trace_ao_inst(case.oview, w, h, dc.dp, ids, sem=SEM, frame=FRAME + f, ao_eps=EPS) for f in range(2)]
    assert np.isposinf(want[0][0]["t"][dc.miss_px]).all() and (want[0][0]["prim"][dc.miss_px] == INVALID).all()
    assert (want[0][1][dc.miss_px] == INVALID).all()

    def expected(frames):
        rec = np.full((frames * n + SLACK, 2), FILL32, dtype=np.uint32)
        ins = np.full(frames * n + SLACK, FILL32, dtype=np.uint32)
        for f in range(frames):
            rec[f * n:(f + 1) * n] = want[f][0].view(np.uint32).reshape(-1, 2)
            if dc.tlas:                                   # (a single-level pass writes no instance ids)
                ins[f * n:(f + 1) * n] = want[f][1]
        return rec, ins

    def launch(kind, d_prim, d_inst, frames=1):
        d_ao, d_ai = _buf((frames * n + SLACK) * 8), _buf((frames * n + SLACK) * 4)
        _sync()
        p = lambda t: C.c_void_p(t.data_ptr())
        with limit():
            if kind == "ao":
                sc.trace_ao_dev(case.view, w, h, d_prim.data_ptr(), d_ao.data_ptr(), sem=SEM, frame=FRAME, ao_eps=EPS)
            elif kind == "inst":
                L.check(sc._lib.trx_trace_ao_inst_dev(sc.handle, C.byref(case.view), w, h, L.Shard(0, 1, 0, 0), SEM, FRAME, EPS, p(d_prim), p(d_inst),
                                                      p(d_ao), p(d_ai), None))
            elif kind == "masked":
                sc.trace_ao_masked_dev(case.view, w, h, d_prim.data_ptr(), d_ao.data_ptr(), 0xFF, sem=SEM, frame=FRAME, ao_eps=EPS,
                                       d_primary_inst=d_inst.data_ptr(), d_ao_inst=d_ai.data_ptr())
            else:
                sc.trace_ao_batch_dev(case.view, w, h, d_prim.data_ptr(), d_ao.data_ptr(), n, frames, sem=SEM, frame0=FRAME, ao_eps=EPS,
                                      d_primary_inst=d_inst.data_ptr(), d_ao_inst=d_ai.data_ptr())
            torch.cuda.synchronize()
        return d_ao.cpu().numpy().view(np.uint32).reshape(-1, 2), d_ai.cpu().numpy().view(np.uint32)

    for kind, frames in (("inst", 1), ("masked", 1), ("batch", 2)) + (() if case.transformed else (("ao", 1),)):
        what = "%s trx_trace_ao_%s" % (case.name, kind)
        (rec, ins), (crec, cins) = dc.both(lambda a, b: launch(kind, a, b, frames))
        wrec, wins = expected(frames)
        _same(rec, wrec, what + " records")
        if kind != "ao":
            _same(ins, wins, what + " instance ids")
        keep = np.concatenate([np.tile(dc.clean, frames), np.ones(SLACK, dtype=bool)])
        _same(rec[keep], crec[keep], what + ": undoctored records against the clean run")
        _same(ins[keep], cins[keep], what + ": undoctored ids against the clean run")
    if not case.transformed:                                 # (the counting forms take no instance ids: refused with rows)
        def count(d_prim, _):
            d_ao, d_cost = _buf((n + SLACK) * 8), _buf((n + SLACK) * 4)
            _sync()
            with limit():
                st = sc.count_ao(case.view, w, h, d_prim.data_ptr(), d_ao.data_ptr(), sem=SEM, frame=FRAME, ao_eps=EPS)
                st2 = sc.count_ao_per_ray(case.view, w, h, d_prim.data_ptr(), d_cost.data_ptr(), d_ao.data_ptr(), sem=SEM, frame=FRAME, ao_eps=EPS)
                torch.cuda.synchronize()
            return st, st2, d_ao.cpu().numpy().view(np.uint32).reshape(-1, 2), d_cost.cpu().numpy().view(np.uint32)
        (st, st2, rec, cost), (cst, _, crec, ccost) = dc.both(count)
        ost, what = want[0][2], case.name + " counting forms"
        six = lambda s: (int(s.n_rays), int(s.n_node), int(s.n_tri), int(s.n_hits), int(s.max_stack), int(s.overflow))
        print(what, "gpu", six(st), "oracle", six(ost), "clean", six(cst))
        assert six(st) == six(ost) and six(st2) == six(ost), what
        _same(rec, expected(1)[0], what + " records")
        assert (cost[n:] == FILL32).all() and (cost[:n][dc.miss_px] == 0).all(), what
        _same(cost[:n][dc.clean], ccost[:n][dc.clean], what + ": undoctored per-ray counts against the clean run")
        pr, cpr = cost[:n].view(COST_DTYPE), ccost[:n].view(COST_DTYPE)
        for field, total, ctotal in (("n_node", st.n_node, cst.n_node), ("n_tri", st.n_tri, cst.n_tri)):
            assert int(pr[field].sum(dtype=np.int64)) == int(total), what
            # the totals move by exactly what the doctored pixels' own rays cost in either run
            assert int(total) - int(ctotal) == int(pr[field][dc.pixels].sum(dtype=np.int64)) - int(cpr[field][dc.pixels].sum(dtype=np.int64)), what
    dc.finish()


# ---- the ray writers (trx_ao_rays_dev, trx_light_rays_dev) ------------------------------------------------------------------------

def _ray_writers(dc):
    torch = _torch()
    case, sc, n, w, h = dc.case, dc.case.sc, dc.n, dc.w, dc.h
    twin, surface = dc.twin("ao_rays", lambda: ao_rays(dc.orc, dc.osc, case.oview, w, h, dc.dp, dc.di, FRAME, EPS, 1.4))
    assert not surface[dc.miss_px].any() and (twin.view(np.uint32).reshape(-1, 8)[dc.miss_px] == INERT).all()

    def ao(d_prim, d_inst):
        d_rays = _buf((n + 2) * 32, 0xA5)
        _sync()
        with limit():
            sc.ao_rays_dev(case.view, w, h, d_prim.data_ptr(), d_rays.data_ptr() + 32, 1.4, frame=FRAME, ao_eps=EPS, d_primary_inst=d_inst.data_ptr())
            torch.cuda.synchronize()
        return d_rays.cpu().numpy().view(np.uint32).reshape(n + 2, 8)
    got, clean = dc.both(ao)
    want = np.full((n + 2, 8), 0xA5A5A5A5, dtype=np.uint32)
    want[1:-1] = twin.view(np.uint32).reshape(-1, 8)
    if case.base is not None:
        padded = np.flatnonzero(surface & (dc.dp["prim"] >= case.osc.tris.shape[0]))   # surface records naming an appended triangle
        assert padded.size >= 4
        got, want = _nan_words(got, want, 1 + padded, case.name + " trx_ao_rays_dev")
    _same(got, want, case.name + " trx_ao_rays_dev")
    _same(got[1:-1][dc.clean], clean[1:-1][dc.clean], case.name + " trx_ao_rays_dev: undoctored rays against the clean run")
    geo = dc.twin("geo", lambda: LT.frame_geometry(case.view, w, h, dc.dp, dc.di, dc.recs, dc.w2o))
    for k, light in enumerate(_mixed(3)):
        def rays(d_prim, d_inst):
            d_rays = _buf((n + 2) * 32, 0xA5)
            _sync()
            with limit():
                sc.light_rays_dev(case.view, w, h, light.product(dc.trx), d_prim.data_ptr(), d_rays.data_ptr() + 32, light_index=k, frame0=FRAME,
                                  sample=k, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                torch.cuda.synchronize()
            return d_rays.cpu().numpy().view(np.uint32).reshape(n + 2, 8)
        got, clean = dc.both(rays)
        twin, cast = LT.light_rays(dc.orc, case.view, w, h, geo, light, k, FRAME, k, EPS)
        assert not cast[dc.miss_px].any()
        want[1:-1] = twin.view(np.uint32).reshape(-1, 8)
        what = "%s trx_light_rays_dev light %d" % (case.name, k)
        _same(got, want, what)
        assert (got[1:-1][dc.miss_px] == INERT).all(), what
        _same(got[1:-1][dc.clean], clean[1:-1][dc.clean], what + ": undoctored rays against the clean run")
    dc.finish()


# ---- the visibility passes (trx_trace_ao_visibility_dev, _sparse_dev, trx_trace_light_visibility_dev) -----------------------------

def _two_chunks(dc, unit, n_samples):
    """A scratch cap under which the pass's samples run in two chunks (all tiles, two samples, then the rest)."""
    tiles = ((dc.w + 7) // 8) * ((dc.h + 7) // 8)
    assert n_samples == 3
    dc.trx.load().trx_debug_ao_scratch_cap(unit * tiles * 2)


def _visibility(dc):
    torch = _torch()
    case, sc, n, w, h, radius = dc.case, dc.case.sc, dc.n, dc.w, dc.h, dc.case.radius
    counts = dc.twin("counts", lambda: visibility_counts(dc.orc, dc.osc, case.oview, w, h, dc.dp, dc.di, SEM, FRAME, 3, EPS, radius))
    assert (counts[dc.miss_px] == NO_SURFACE).all() and (counts[dc.pixels[dc.is_surface]] <= 3).all()
    try:
        _two_chunks(dc, UNIT, 3)

        def dense(d_prim, d_inst):
            d_out = _buf(n + 64)
            _sync()
            with limit():
                sc.trace_ao_visibility_dev(case.view, w, h, d_prim.data_ptr(), d_out.data_ptr(), 3, radius, sem=SEM, frame0=FRAME, ao_eps=EPS,
                                           d_primary_inst=d_inst.data_ptr())
                torch.cuda.synchronize()
            return d_out.cpu().numpy()
        got, clean = dc.both(dense)
        _same(got, np.concatenate([counts, np.full(64, FILL, dtype=np.uint8)]), case.name + " trx_trace_ao_visibility_dev")
        _same(got[:n][dc.clean], clean[:n][dc.clean], case.name + " trx_trace_ao_visibility_dev: undoctored counts against the clean run")
        for phase in (0, 3):
            wlo, hlo = lo_size(w, h, 2)

            def sparse(d_prim, d_inst):
                d_out = _buf(wlo * hlo + 64)
                _sync()
                with limit():
                    sc.trace_ao_visibility_sparse_dev(case.view, w, h, 2, phase, d_prim.data_ptr(), d_out.data_ptr(), 3, radius, sem=SEM, frame0=FRAME,
                                                      ao_eps=EPS, d_primary_inst=d_inst.data_ptr())
                    torch.cuda.synchronize()
                return d_out.cpu().numpy()
            got, clean = dc.both(sparse)
            what = "%s trx_trace_ao_visibility_sparse_dev phase %d" % (case.name, phase)
            _same(got, np.concatenate([sparse_counts(counts, w, h, 2, phase), np.full(64, FILL, dtype=np.uint8)]), what)
            gx, gy, inside = cell_pixels(w, h, 2, phase)
            keep = (~inside | dc.clean[np.minimum(gy, h - 1) * w + np.minimum(gx, w - 1)]).reshape(-1)
            _same(got[:wlo * hlo][keep], clean[:wlo * hlo][keep], what + ": undoctored cells against the clean run")
        lights = _mixed(3)
        geo = dc.twin("geo", lambda: LT.frame_geometry(case.view, w, h, dc.dp, dc.di, dc.recs, dc.w2o))
        planes = LT.visibility_planes(dc.orc, dc.osc, case.view, w, h, geo, dc.dp, lights, FRAME, 3, EPS, SEM)
        assert (planes[:, dc.miss_px] == NO_SURFACE).all()

        def lit(d_prim, d_inst):
            d_out = _buf(3 * n + 64)
            _sync()
            with limit():
                sc.trace_light_visibility_dev(case.view, w, h, [l.product(dc.trx) for l in lights], d_prim.data_ptr(), d_out.data_ptr(), n_samples=3,
                                              sem=SEM, frame0=FRAME, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                torch.cuda.synchronize()
            return d_out.cpu().numpy()
        got, clean = dc.both(lit)
        _same(got, np.concatenate([planes.reshape(-1), np.full(64, FILL, dtype=np.uint8)]), case.name + " trx_trace_light_visibility_dev")
        keep = np.tile(dc.clean, 3)
        _same(got[:3 * n][keep], clean[:3 * n][keep], case.name + " trx_trace_light_visibility_dev: undoctored counts against the clean run")
    finally:
        dc.trx.load().trx_debug_ao_scratch_cap(0)
    dc.finish()


# ---- the indirect passes (trx_trace_indirect_dev, _sparse_dev) --------------------------------------------------------------------

def _indirect(dc):
    torch = _torch()
    case, sc, n, w, h = dc.case, dc.case.sc, dc.n, dc.w, dc.h
    lights = _mixed(2)
    base = np.random.default_rng(7).random(n).astype(np.float32)
    base[dc.miss_px[0::2]] = f32(-0.0)                       # a miss keeps its base's bits: -0, and a NaN with a payload
    base.view(np.uint32)[dc.miss_px[1::2]] = 0x7FC12345
    args = (dc.recs, dc.w2o, lights, FRAME, 2, EPS, EPS, ALBEDO, SEM)
    cache = {}
    with_base = IT.indirect(dc.orc, dc.osc, case.oview, w, h, dc.dp, dc.di, *args, base=base, cache=cache)
    without = IT.indirect(dc.orc, dc.osc, case.oview, w, h, dc.dp, dc.di, *args, cache=cache)
    assert (with_base.view(np.uint32)[dc.miss_px] == base.view(np.uint32)[dc.miss_px]).all() and (without.view(np.uint32)[dc.miss_px] == 0).all()
    prods = [l.product(dc.trx) for l in lights]
    try:
        dc.trx.load().trx_debug_ao_scratch_cap(GI_UNIT * ((w + 7) // 8) * ((h + 7) // 8))          # (one sample per chunk: two chunks)

        def dense(d_prim, d_inst):
            d_out, d_base = _buf(n * 4 + 64), _dev(base)
            _sync()
            with limit():
                sc.trace_indirect_dev(case.view, w, h, prods, d_prim.data_ptr(), d_out.data_ptr(), n_samples=2, sem=SEM, frame0=FRAME, bounce_eps=EPS,
                                      shadow_eps=EPS, bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr(), d_base=d_base.data_ptr())
                torch.cuda.synchronize()
            return d_out.cpu().numpy()
        got, clean = dc.both(dense)
        _same(got, np.concatenate([with_base.view(np.uint8), np.full(64, FILL, dtype=np.uint8)]), case.name + " trx_trace_indirect_dev")
        keep = np.repeat(dc.clean, 4)
        _same(got[:4 * n][keep], clean[:4 * n][keep], case.name + " trx_trace_indirect_dev: undoctored values against the clean run")
        for phase in (0, 3):
            wlo, hlo = lo_size(w, h, 2)

            def sparse(d_prim, d_inst):
                d_out = _buf(wlo * hlo * 4 + 64)
                _sync()
                with limit():
                    sc.trace_indirect_sparse_dev(case.view, w, h, 2, phase, prods, d_prim.data_ptr(), d_out.data_ptr(), n_samples=2, sem=SEM, frame0=FRAME,
                                                 bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr())
                    torch.cuda.synchronize()
                return d_out.cpu().numpy()
            got, clean = dc.both(sparse)
            what = "%s trx_trace_indirect_sparse_dev phase %d" % (case.name, phase)
            lo = IST.sparse_values(without, dc.dp, w, h, 2, phase, n_tris=dc.n_tris)
            _same(got, np.concatenate([lo.view(np.uint8), np.full(64, FILL, dtype=np.uint8)]), what)
            gx, gy, inside = cell_pixels(w, h, 2, phase)
            keep = np.repeat((~inside | dc.clean[np.minimum(gy, h - 1) * w + np.minimum(gx, w - 1)]).reshape(-1), 4)
            _same(got[:wlo * hlo * 4][keep], clean[:wlo * hlo * 4][keep], what + ": undoctored cells against the clean run")
    finally:
        dc.trx.load().trx_debug_ao_scratch_cap(0)
    dc.finish()


# ---- the tests, the ids just past the tables first ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_ids_just_past_the_tables_ao_passes(cases, name):
    _ao_passes(cases(name, True))


@pytest.mark.parametrize("name", CASES)
def test_ids_just_past_the_tables_ray_writers(cases, name):
    _ray_writers(cases(name, True))


@pytest.mark.parametrize("name", CASES)
def test_ids_just_past_the_tables_visibility_passes(cases, name):
    _visibility(cases(name, True))


@pytest.mark.parametrize("name", CASES)
def test_ids_just_past_the_tables_indirect_passes(cases, name):
    _indirect(cases(name, True))


@pytest.mark.parametrize("name", CASES)
def test_the_whole_table_ao_passes(cases, name):
    """2^31, 0xFFFFFFFE, and 0x55555556 / 0xAAAAAAAB, whose triple wraps 32 bits to 2 and 1, among the ids."""
    _ao_passes(cases(name, False))


@pytest.mark.parametrize("name", CASES)
def test_the_whole_table_ray_writers(cases, name):
    _ray_writers(cases(name, False))


@pytest.mark.parametrize("name", CASES)
def test_the_whole_table_visibility_passes(cases, name):
    _visibility(cases(name, False))


@pytest.mark.parametrize("name", CASES)
def test_the_whole_table_indirect_passes(cases, name):
    _indirect(cases(name, False))


# ---- the sentinel frame -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "instanced"])
def test_a_shard_traced_into_a_sentinel_frame_leaves_the_other_shards_misses(trx, orc, cases, name):
    """Shard (1, 3) of the primary frame in image layout, traced into buffers filled with the suite's sentinel byte - the other
    shards' records are {t = 1.5e16, prim = 0x5A5A5A5A} beside the id 0x5A5A5A5A - then the whole-image passes over it: sparse AO
    visibility and its upsample, the sparse indirect pass and trx_value_upsample_dev, against the twins over the same bytes."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    dc = cases(name, True)
    case, sc, n, w, h = dc.case, dc.case.sc, dc.n, dc.w, dc.h
    d_prim, d_inst = _buf(n * 8), _buf(n * 4)
    _sync()
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(case.view), w, h, L.Shard(1, 3, 0, 0), SEM, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        torch.cuda.synchronize()
    prim, inst = d_prim.cpu().numpy().view(orc.HIT_DTYPE).copy(), d_inst.cpu().numpy().view(np.uint32).copy()
    mine, _, _ = record_map(w, h, (1, 3, 0))
    other = np.ones(n, dtype=bool)
    other[mine] = False
    assert (prim["prim"][other] == FILL32).all() and (prim["t"][other] < LT.F32_MAX).all() and (prim.view(np.uint32).reshape(-1, 2)[mine] != FILL32).any(1).all()
    assert dc.n_tris <= FILL32 and other.sum() > n // 2 and surface_records(prim, dc.n_tris)[mine].sum() >= 100     # (the shard's own surface: a third of the frame's)
    ids = inst if dc.tlas else None
    counts = visibility_counts(orc, dc.osc, case.oview, w, h, prim, ids, SEM, FRAME, 3, EPS, case.radius)
    assert (counts[other] == NO_SURFACE).all()
    lights = _mixed(2)
    values = IT.indirect(orc, dc.osc, case.oview, w, h, prim, ids, dc.recs, dc.w2o, lights, FRAME, 2, EPS, EPS, ALBEDO, SEM)
    assert (values.view(np.uint32)[other] == 0).all() and (values[mine] > 0).any()
    wlo, hlo = lo_size(w, h, 2)
    for phase in (0, 3):
        what = "%s phase %d" % (name, phase)
        gx, gy, inside = cell_pixels(w, h, 2, phase)
        cell_other = (inside & other[np.minimum(gy, h - 1) * w + np.minimum(gx, w - 1)]).reshape(-1)
        assert cell_other.any()
        d_lo, d_term, d_vlo, d_val = _buf(wlo * hlo + 64), _buf(n * 4 + 64), _buf(wlo * hlo * 4 + 64), _buf(n * 4 + 64)
        _sync()
        with limit():
            sc.trace_ao_visibility_sparse_dev(case.view, w, h, 2, phase, d_prim.data_ptr(), d_lo.data_ptr(), 3, case.radius, sem=SEM, frame0=FRAME,
                                              ao_eps=EPS, d_primary_inst=d_inst.data_ptr())
            sc.ao_upsample_dev(w, h, 2, phase, d_prim.data_ptr(), d_lo.data_ptr(), d_term.data_ptr(), 3, 1)
            sc.trace_indirect_sparse_dev(case.view, w, h, 2, phase, [l.product(trx) for l in lights], d_prim.data_ptr(), d_vlo.data_ptr(), n_samples=2,
                                         sem=SEM, frame0=FRAME, bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr())
            sc.value_upsample_dev(w, h, 2, phase, d_prim.data_ptr(), d_vlo.data_ptr(), d_val.data_ptr(), 1)
            torch.cuda.synchronize()
            sc.check()
        tail = np.full(64, FILL, dtype=np.uint8)
        lo = sparse_counts(counts, w, h, 2, phase)
        got_lo = d_lo.cpu().numpy()
        _same(got_lo, np.concatenate([lo, tail]), what + " sparse AO visibility")
        assert (got_lo[:wlo * hlo][cell_other] == NO_SURFACE).all(), what
        term = ao_upsample(prim, None, lo, w, h, 2, phase, 3, 1, 0.02, 0.9)
        _same(d_term.cpu().numpy(), np.concatenate([term.view(np.uint8), tail]), what + " AO upsample")
        vlo = IST.sparse_values(values, prim, w, h, 2, phase, n_tris=dc.n_tris)
        got_vlo = d_vlo.cpu().numpy()
        _same(got_vlo, np.concatenate([vlo.view(np.uint8), tail]), what + " sparse indirect")
        assert (got_vlo[:wlo * hlo * 4].view(np.uint32)[cell_other] == 0).all(), what
        up = IST.value_upsample(prim, None, vlo, w, h, 2, phase, 1, 0.1, 0.9)
        _same(d_val.cpu().numpy(), np.concatenate([up.view(np.uint8), tail]), what + " value upsample")
    assert TERM_DTYPE.itemsize == 4
    dc.finish()
