"""Caller records on the CPU (include/trx.h, "CALLER RECORDS"): the oracle's orc_ao_ray_inst, its AO loops and every numpy
twin of a pass that indexes the scene's tables with a caller's record, over the record table of tests/caller_records.py -
every t crossed with every prim (and every instance id) at, just past and far past the tables' ends.

What is expected is written out by hand: the table's columns say which entries are surface records and which ids select a
row; a miss gives the literal miss outputs; a surface record gives what its canonical record gives - the same t and prim
beside an id that every pass understood before the rule was stated.  A stand-alone C program walks the same table through
orc_ao_ray_inst under AddressSanitizer and UBSan, with tables that end exactly where the scene says."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ao_sparse_twin as AST
import indirect_sparse_twin as IST
import indirect_twin as IT
import light_twin as LT
from ao_visibility_twin import NO_SURFACE, ao_rays, golden_case, instanced_case, surface_records, visibility_counts
from caller_records import FLT_MAX, INVALID, OWN, T_TABLE, TILE, doctor, entries, inst_table, pick_pixels, prim_table
from hit_attr_twin import tri_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.01
INERT = np.array([0, 0, 0, 0, 0, 0, 0, 0xBF800000], dtype=np.uint32)
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Frame:
    """A scene of the suite on the oracle, its own primary frame, and that frame doctored with the whole table."""

    def __init__(self, trx, orc, name):
        self.orc = orc
        if name == "instanced":
            _, self.view, self.osc, self.oview, self.w, self.h = instanced_case(trx, orc)
        else:
            self.osc, self.oview, self.w, self.h, _ = golden_case(trx, orc, name)
            self.view = self.oview
        self.w2o = self.osc.w2o
        self.n_tris, self.n_inst = self.osc.tris.shape[0], int(self.osc.inst.size)
        self.recs = tri_records(self.osc.verts)
        self.prim, inst, _ = self.osc.trace_primary_inst(self.oview, self.w, self.h, sem=0)
        self.inst = inst if self.n_inst else None
        self.table = entries(self.n_tris, self.n_inst)
        self.pixels, self.tile = pick_pixels(self.w, self.h, len(self.table), surface_records(self.prim, self.n_tris))
        self.dp, self.di, self.cp, self.ci, self.is_surface = doctor(self.prim, self.inst, self.pixels, self.table)
        self.miss_px, self.surf_px = self.pixels[~self.is_surface], self.pixels[self.is_surface]


@pytest.fixture(scope="module")
def frames(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Frame(trx, orc, name)
        return made[name]
    return get


SCENES = ["cornell_64", "instanced"]


def test_the_table_is_the_issues_table():
    assert [t for t, _ in T_TABLE[1:4]] == [1.0, -1.0, 0.0] and T_TABLE[0][0] is OWN
    assert T_TABLE[4][0].view(np.uint32) == 0x7F7FFFFE and T_TABLE[5][0] == FLT_MAX and np.isinf(T_TABLE[6][0]) and np.isnan(T_TABLE[7][0])
    assert [ok for _, ok in T_TABLE[1:]] == [True, True, True, True, False, False, False]
    assert [p for p, _ in prim_table(100)] == [0, 99, 100, 101, 2 ** 31, 0x55555556, 0xAAAAAAAB, 0xFFFFFFFE, 0xFFFFFFFF]
    assert [ok for _, ok in prim_table(100)] == [True, True] + [False] * 7
    assert [i for i, _ in inst_table(14)] == [0, 13, 14, 15, 2 ** 31, 0xFFFFFFFE, 0xFFFFFFFF]
    assert [ok for _, ok in inst_table(14)] == [True, True] + [False] * 5
    assert (3 * 0x55555556) & 0xFFFFFFFF == 2 and (3 * 0xAAAAAAAB) & 0xFFFFFFFF == 1     # (why these two are in the table)
    assert len(entries(100)) == 72 and len(entries(100, 14)) == 504


@pytest.mark.parametrize("name", SCENES)
def test_the_doctored_frame_holds_every_entry_in_every_group(frames, name):
    fr = frames(name)
    assert len(fr.pixels) - TILE >= len(fr.table) and np.unique(fr.pixels).size == len(fr.pixels)
    assert fr.tile.size == TILE and (fr.pixels[:TILE] == fr.tile).all() and 0 in fr.pixels and fr.w * fr.h - 1 in fr.pixels
    # the whole tile: not one surface record, and both kinds of miss - a prim past the table beside a usable t, and the reverse
    assert not fr.is_surface[:TILE].any() and not surface_records(fr.dp, fr.n_tris)[fr.tile].any()
    assert ((fr.dp["t"][fr.tile] < FLT_MAX) & (fr.dp["prim"][fr.tile] >= fr.n_tris)).any()
    assert (~(fr.dp["t"][fr.tile] < FLT_MAX) & (fr.dp["prim"][fr.tile] < fr.n_tris)).any()
    assert surface_records(fr.prim, fr.n_tris)[fr.tile].sum() >= 32          # (it was a tile of surface pixels)
    assert 0 < fr.surf_px.size < len(fr.pixels)
    clean = np.ones(fr.w * fr.h, dtype=bool)
    clean[fr.pixels] = False
    assert (clean & surface_records(fr.prim, fr.n_tris)).sum() >= 200
    # the canonical records are records every pass took before: a miss, or a prim inside the table beside an id that selects a row or 0xFFFFFFFF
    assert ((fr.cp["prim"] < fr.n_tris) | ((fr.cp["prim"] == INVALID) & np.isinf(fr.cp["t"]))).all()
    if fr.ci is not None:
        assert ((fr.ci < fr.n_inst) | (fr.ci == INVALID)).all()


@pytest.mark.parametrize("name", SCENES)
def test_orc_ao_ray_inst_follows_the_rule_entry_by_entry(orc, frames, name):
    """The return value is the table's column; a surface record's origin is (eye + d * t) - d * eps of ITS t in binary32, its
    direction that of the plain record {1.0, prim} beside the id where it selects a row and beside 0xFFFFFFFF where not."""
    fr = frames(name)
    lib = orc.load()
    sc, vw = C.byref(fr.osc.c), C.byref(fr.oview)
    eye = np.array(fr.oview.eye, dtype=np.float32)

    def call(i, t, p, ii):
        o, d = np.full(3, 7.0, dtype=np.float32), np.full(3, 7.0, dtype=np.float32)
        ok = lib.orc_ao_ray_inst(sc, vw, fr.w, fr.h, int(i % fr.w), int(i // fr.w), orc.HitC(float(t), int(p)), int(ii), 3, EPS,
                                 o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
        return ok, o, d

    n_surface = 0
    for k, i in enumerate(fr.pixels):
        if k < TILE:
            continue                                                  # (the whole tile holds misses only: the entries follow it)
        t, t_ok, p, p_ok, ii, i_ok = fr.table[(k - TILE) % len(fr.table)]
        if t is OWN:
            t, t_ok = fr.prim["t"][i], bool(np.isfinite(fr.prim["t"][i]))
        ok, o, d = call(i, t, p, ii)
        what = "%s pixel %d: t %r prim 0x%08x inst 0x%08x" % (name, i, t, p, ii)
        assert ok == int(t_ok and p_ok), what
        if not ok:
            continue
        n_surface += 1
        ro, rd = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        lib.orc_primary_ray(vw, fr.w, fr.h, int(i % fr.w), int(i // fr.w), ro.ctypes.data_as(C.c_void_p), rd.ctypes.data_as(C.c_void_p))
        with np.errstate(over="ignore", invalid="ignore"):
            want_o = ((eye + rd * f32(t)) - rd * f32(EPS)).astype(np.float32)
        assert (o.view(np.uint32) == want_o.view(np.uint32)).all(), what
        ok2, _, d2 = call(i, 1.0, p, ii if i_ok else INVALID)
        assert ok2 == 1 and (d.view(np.uint32) == d2.view(np.uint32)).all(), what
        # ... and, by hand from the triangle's record: a unit vector in the hemisphere of the normal flipped toward the viewer -
        # the object-space normal through the id's row where it selects one, as it is where it selects none
        nrm = fr.recs[p, 9:12].astype(np.float64)
        if fr.w2o is not None and i_ok:
            m = fr.w2o[ii].astype(np.float64)
            nrm = np.array([m[c] * nrm[0] + m[4 + c] * nrm[1] + m[8 + c] * nrm[2] for c in range(3)])
        nrm = nrm / np.linalg.norm(nrm)
        nrm = nrm if nrm @ -rd.astype(np.float64) >= 0 else -nrm
        assert abs(np.linalg.norm(d.astype(np.float64)) - 1) < 1e-6 and d.astype(np.float64) @ nrm > -1e-6, what
    assert n_surface >= 8                                             # (1, -1, +0 and 0x7F7FFFFE beside prim 0 and n_tris - 1, at the least)


@pytest.mark.parametrize("name", SCENES)
def test_the_oracles_ao_loops_give_the_canonical_answers(orc, frames, name):
    """trace_ao (scenes without rows), trace_ao_inst and orc_ao_rays over the doctored frame: the records, ids, rays and
    counters of the canonical frame, bit for bit; the doctored misses are {+inf, 0xFFFFFFFF}, id 0xFFFFFFFF and the inert ray."""
    fr = frames(name)
    for sem, frame in ((0, 0), (3, 5)):
        if fr.w2o is None:
            got, st = fr.osc.trace_ao(fr.oview, fr.w, fr.h, fr.dp, sem=sem, frame=frame, ao_eps=EPS)
            want, wst = fr.osc.trace_ao(fr.oview, fr.w, fr.h, fr.cp, sem=sem, frame=frame, ao_eps=EPS)
            assert (_bits(got) == _bits(want)).all() and _six(st) == _six(wst)
        no_ids = np.full(fr.w * fr.h, INVALID, dtype=np.uint32)
        got, gi, st = fr.osc.trace_ao_inst(fr.oview, fr.w, fr.h, fr.dp, fr.di if fr.di is not None else no_ids, sem=sem, frame=frame, ao_eps=EPS)
        want, wi, wst = fr.osc.trace_ao_inst(fr.oview, fr.w, fr.h, fr.cp, fr.ci if fr.ci is not None else no_ids, sem=sem, frame=frame, ao_eps=EPS)
        assert (_bits(got) == _bits(want)).all() and (gi == wi).all() and _six(st) == _six(wst)
        assert np.isposinf(got["t"][fr.miss_px]).all() and (got["prim"][fr.miss_px] == INVALID).all() and (gi[fr.miss_px] == INVALID).all()
        assert st.n_rays == surface_records(fr.cp, fr.n_tris).sum()
        rays = fr.osc.ao_rays(fr.oview, fr.w, fr.h, fr.dp, fr.di, frame=frame, ao_eps=EPS, tmax=1.5)
        want = fr.osc.ao_rays(fr.oview, fr.w, fr.h, fr.cp, fr.ci, frame=frame, ao_eps=EPS, tmax=1.5)
        assert (_bits(rays) == _bits(want)).all()
        assert (rays.view(np.uint32).reshape(-1, 8)[fr.miss_px] == INERT).all()
        assert (rays["tmax"][fr.surf_px] == f32(1.5)).all()


def _six(st):
    return (int(st.n_rays), int(st.n_node), int(st.n_tri), int(st.n_hits), int(st.max_stack), int(st.overflow))


@pytest.mark.parametrize("name", SCENES)
def test_the_visibility_twins_give_the_canonical_answers(orc, frames, name):
    """ao_visibility_twin (rays, counts), ao_sparse_twin's subsampling of them, and light_twin (geometry, rays, planes)."""
    fr = frames(name)
    rays, surf = ao_rays(orc, fr.osc, fr.oview, fr.w, fr.h, fr.dp, fr.di, 4, EPS, 1.4)
    want, wsurf = ao_rays(orc, fr.osc, fr.oview, fr.w, fr.h, fr.cp, fr.ci, 4, EPS, 1.4)
    assert (_bits(rays) == _bits(want)).all() and (surf == wsurf).all()
    assert not surf[fr.miss_px].any() and surf[fr.surf_px].all()
    assert (rays.view(np.uint32).reshape(-1, 8)[fr.miss_px] == INERT).all()
    counts = visibility_counts(orc, fr.osc, fr.oview, fr.w, fr.h, fr.dp, fr.di, 0, 2, 2, EPS, 1.4)
    assert (counts == visibility_counts(orc, fr.osc, fr.oview, fr.w, fr.h, fr.cp, fr.ci, 0, 2, 2, EPS, 1.4)).all()
    assert (counts[fr.miss_px] == NO_SURFACE).all() and (counts[fr.surf_px] <= 2).all()
    for phase in (0, 3):
        lo = AST.sparse_counts(counts, fr.w, fr.h, 2, phase).reshape(AST.lo_size(fr.w, fr.h, 2)[::-1])
        gx, gy, inside = AST.cell_pixels(fr.w, fr.h, 2, phase)
        on = np.isin(gy * fr.w + gx, fr.miss_px) & inside
        assert on.any() and (lo[on] == NO_SURFACE).all()              # (doctored misses on this phase's grid)
    # the light twin
    geo = LT.frame_geometry(fr.view, fr.w, fr.h, fr.dp, fr.di, fr.recs, fr.w2o)
    wgeo = LT.frame_geometry(fr.view, fr.w, fr.h, fr.cp, fr.ci, fr.recs, fr.w2o)
    assert (geo[0] == np.flatnonzero(surface_records(fr.cp, fr.n_tris))).all()
    if fr.w2o is None:
        for a, b in zip(geo, wgeo):
            assert (_bits(a) == _bits(b)).all()
    else:
        # an id that selects no row: the unit object-space normal, flipped toward the viewer - by hand from the triangle's record
        for a, b in zip(geo[:4] + geo[5:], wgeo[:4] + wgeo[5:]):
            assert (_bits(a) == _bits(b)).all()
        ids = fr.di[geo[0]]
        no_row = ids >= fr.n_inst
        assert no_row.sum() >= 10 and (~no_row).sum() >= 200
        ng = fr.recs[fr.dp["prim"][geo[0]][no_row], 9:12]
        unit = (ng * (f32(1.0) / np.sqrt((ng[:, 0] * ng[:, 0] + ng[:, 1] * ng[:, 1]) + ng[:, 2] * ng[:, 2]))[:, None]).astype(np.float32)
        assert (_bits(geo[4][no_row]) == _bits(LT.flip(unit, geo[3][no_row]))).all()
        assert (_bits(geo[4][~no_row]) == _bits(wgeo[4][~no_row])).all()
        wgeo = geo                                                    # (from here on: one geometry, checked above)
    lights = [LT.Light(LT.POINT, (0.0, 1.8, 0.0)), LT.RECT_CASE, LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.4))]
    for k, light in enumerate(lights):
        r, cast = LT.light_rays(orc, fr.view, fr.w, fr.h, geo, light, k, 0, 1, EPS)
        assert not cast[fr.miss_px].any() and (r.view(np.uint32).reshape(-1, 8)[fr.miss_px] == INERT).all()
    planes = LT.visibility_planes(orc, fr.osc, fr.view, fr.w, fr.h, geo, fr.dp, lights, 0, 2, EPS, 0)
    assert (planes[:, fr.miss_px] == NO_SURFACE).all() and (planes[:, fr.surf_px] != NO_SURFACE).all()
    if fr.w2o is None:
        assert (planes == LT.visibility_planes(orc, fr.osc, fr.view, fr.w, fr.h, wgeo, fr.cp, lights, 0, 2, EPS, 0)).all()
    # the light term reads no scene table: it keeps prim != 0xFFFFFFFF
    assert (LT.surface(fr.dp) == ((fr.dp["t"] < FLT_MAX) & (fr.dp["prim"] != INVALID))).all()
    assert (LT.surface(fr.dp) & ~LT.surface(fr.dp, fr.n_tris)).sum() >= 10


@pytest.mark.parametrize("name", SCENES)
def test_the_indirect_twins_give_the_canonical_answers(orc, frames, name):
    """indirect_twin over the doctored frame, with a base whose bits a miss must keep (-0.0, a NaN with a payload), and
    indirect_sparse_twin's subsampling under the scene's rule."""
    fr = frames(name)
    lights = [LT.Light(LT.POINT, (0.0, 1.8, 0.0), intensity=1.5), LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5)]
    base = np.random.default_rng(2).random(fr.w * fr.h).astype(np.float32)
    base[fr.miss_px[0::2]] = f32(-0.0)
    base.view(np.uint32)[fr.miss_px[1::2]] = 0x7FC12345
    args = (fr.recs, fr.w2o, lights, 1, 2, EPS, EPS, 0.6, 0)
    got = IT.indirect(orc, fr.osc, fr.oview, fr.w, fr.h, fr.dp, fr.di, *args, base=base)
    want = IT.indirect(orc, fr.osc, fr.oview, fr.w, fr.h, fr.cp, fr.ci, *args, base=base)
    assert (_bits(got) == _bits(want)).all()
    assert (got.view(np.uint32)[fr.miss_px] == base.view(np.uint32)[fr.miss_px]).all()
    dense = IT.indirect(orc, fr.osc, fr.oview, fr.w, fr.h, fr.dp, fr.di, *args)
    assert (dense.view(np.uint32)[fr.miss_px] == 0).all() and (dense[fr.surf_px] > 0).any()
    # a pass that believed prim != 0xFFFFFFFF would put a surface pixel's value at the doctored misses' cells
    fake = np.ones(fr.w * fr.h, dtype=np.float32)
    for phase in (0, 3):
        lo = IST.sparse_values(fake, fr.dp, fr.w, fr.h, 2, phase, n_tris=fr.n_tris)
        assert (_bits(lo) == _bits(IST.sparse_values(fake, fr.cp, fr.w, fr.h, 2, phase))).all()
        assert (lo != IST.sparse_values(fake, fr.dp, fr.w, fr.h, 2, phase)).any()


def test_the_table_walk_is_clean_under_the_sanitizers(tmp_path):
    """tests/c_abi/caller_records_walk.c with oracle/trx_oracle.c under -fsanitize=address,undefined, run as a child process:
    tables that end exactly at n_tris and n_instances, every entry of the table, scenes with and without rows."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = tmp_path / "caller_records_walk"
    subprocess.run([cc, "-std=c11", "-O1", "-g", "-fopenmp", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "c_abi", "caller_records_walk.c"), os.path.join(ROOT, "oracle", "trx_oracle.c"), "-o", str(exe), "-lm"],
                   check=True, capture_output=True, timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "1008 calls, 0 wrong" in run.stdout
