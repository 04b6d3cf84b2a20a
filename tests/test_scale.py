"""Power-of-two scene scaling on the CPU: the construction of tests/scale_cases.py is sound before any GPU sees it.

SAFE: for every exponent and every case, each post-walk output of the twins over the carried records is the k = 0 output
under scale_cases.expect_from_base, for every record and with no tolerance.  WALKED: the oracle's primary records over the
rebuilt tree are the k = 0 records under the same table - what licenses the walked GPU cases.  The regime conditions are
computed from the twin here, never from the device: they keep an EDGE case from passing while reaching nothing.  The table of
DESIGN.md ("scene scale") is computed here, and the document is held to it.

Visibility, occlusion and bounce hits depend on a walk and its absolute 0.0001 clamp: they are not asked to be covariant."""
import os

import numpy as np
import pytest

import light_twin as LT
import scale_cases as SC
import scale_twin as ST
from hit_attr_twin import primary_dirs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["%s_%dx%d" % c for c in SC.CASES]


@pytest.fixture(scope="module")
def worlds(trx, orc):
    made = {}

    def get(case):
        if case not in made:
            base = SC.recentred(trx, *case)
            s0, p0 = SC.scaled(trx, base, 0), SC.scaled_params(base, 0)
            f0 = ST.base_frame(orc, s0, p0)
            made[case] = (base, s0, f0, ST.twin_outputs(orc, s0, p0, f0))
        return made[case]
    return get


def _at(trx, orc, world, k):
    base, s0, f0, _ = world
    s, p = SC.scaled(trx, base, k), SC.scaled_params(base, k)
    return s, p, ST.carried_frame(orc, s0, f0, s)


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_the_base_frames_reach_every_output(worlds, case):
    """The k = 0 frame is no empty one: surface pixels, misses, bounce hits and bounce misses, cast and inert rays of every
    writer, emitters, non-zero terms."""
    base, s0, f0, out0 = worlds(case)
    n = s0.w * s0.h
    surf = LT.surface(f0.prim, s0.flat.n_tris)
    assert 100 < surf.sum() < n - 100, surf.sum()
    hit = f0.b_hits["prim"] != SC.INVALID
    assert hit.sum() > 20 and (~hit & surf).sum() > 5
    for name, out in out0.items():
        if "rays" in name:
            cast = out["tmax"] >= 0
            assert cast.sum() > 10 and (~cast).sum() > 10, (name, cast.sum())
    assert out0["selection"]["P"].size >= 2 and (out0["light_term_local"]["term"] > 0).sum() > 50
    assert (out0["emitter_wgeo"]["wgeo"] > 0).sum() > 10 and np.unique(out0["emitter_select"]["j"]).size >= 2
    assert not s0.tlas or np.unique(f0.inst[surf]).size > 2


@pytest.mark.parametrize("k", SC.SAFE)
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_safe_exponents_are_exactly_covariant(trx, orc, worlds, case, k):
    world = worlds(case)
    s, p, f = _at(trx, orc, world, k)
    out = ST.twin_outputs(orc, s, p, f)
    assert set(out) == set(world[3]) and set(out) <= set(SC.RULES)
    for name in out:
        SC.assert_same(out[name], SC.expect_from_base(name, world[3][name], k), "%s k %d %s" % (IDS[SC.CASES.index(case)], k, name))


@pytest.mark.parametrize("k", SC.WALKED)
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_walked_exponents_find_the_base_surface(trx, orc, worlds, case, k):
    """The oracle's own walk over the rebuilt tree at exponent k: t / 2^k, the triangle and the instance of every pixel are
    the k = 0 walk's."""
    base, s0, f0, _ = worlds(case)
    s = SC.scaled(trx, base, k)
    osc = ST.oracle_scene(orc, s)
    prim, inst, _ = osc.trace_primary_inst(orc.view_from_bytes(bytes(s.view)), s.w, s.h)
    got = ST.primary_of(s, prim, inst)
    SC.assert_same(got, SC.expect_from_base("primary", ST.primary_of(s0, f0.prim, f0.inst), k), "%s k %d primary" % (case[0], k))


def test_a_scene_nearer_than_the_clamp_is_all_misses(trx, orc, worlds):
    """At k = -20 the whole Cornell stand-in lies nearer than the node test's max(..., 0.0001): the walk finds nothing - why
    WALKED stops where it does, and what include/trx.h says of it."""
    base, s0, f0, _ = worlds(SC.CASES[0])
    s = SC.scaled(trx, base, -20)
    prim, _, _ = ST.oracle_scene(orc, s).trace_primary_inst(orc.view_from_bytes(bytes(s.view)), s.w, s.h)
    assert (prim["prim"] == SC.INVALID).all() and float(SC.pow2(f0.prim["t"][LT.surface(f0.prim)], -20).max()) < 0.0001


# ---- the regime conditions ------------------------------------------------------------------------------------------------------

def _normals(trx, orc, world, k):
    s, p, f = _at(trx, orc, world, k)
    surf, q = ST.normal_regime(s, f)
    return surf, q, ST.twin_outputs(orc, s, p, f, only={"attr"})["attr"]["normal"][surf], (s, p, f)


def test_regime_denormal_sums(trx, orc, worlds):
    tiny = np.float32(np.finfo(np.float32).tiny)
    found = {}
    for k in SC.EDGE:
        surf, q, _, _ = _normals(trx, orc, worlds(SC.CASES[0]), k)
        found[k] = int(((q > 0) & (q < tiny)).sum())
    assert found[-32] >= 100, found


def test_regime_non_finite_and_zero_normals(trx, orc, worlds):
    world = worlds(SC.CASES[0])
    surf, q, n, _ = _normals(trx, orc, world, -38)
    assert surf.size > 100 and (~np.isfinite(n)).any(1).all(), "k = -38: a surface pixel keeps a finite normal"
    surf, q, n, _ = _normals(trx, orc, world, 48)
    assert surf.size > 100 and (n == 0).all(), "k = +48: a surface pixel keeps a non-zero normal"


def test_regime_overflowing_distance_squares(trx, orc, worlds):
    """k = +68: q = dot(v, v) of the light twin's point and rect lights is +inf at every surface pixel - so at every cast sample.
    (At +62 it is still finite everywhere on this scene: the exponent moved, not the bound.)"""
    world = worlds(SC.CASES[0])
    s, p, f = _at(trx, orc, world, 68)
    surf = np.flatnonzero(LT.surface(f.prim))
    d = primary_dirs(s.view, s.w, s.h, surf % s.w, surf // s.w)
    with np.errstate(over="ignore"):
        P = (d * f.prim["t"][surf][:, None]).astype(np.float32)
        for C in (p.point.position, (p.rect.position + np.float32(0.5) * p.rect.edge1) + np.float32(0.5) * p.rect.edge2):
            v = (C[None, :] - P).astype(np.float32)
            q = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            assert surf.size > 100 and np.isposinf(q).all(), (np.isposinf(q).mean(), q.min())


@pytest.mark.parametrize("k", [-29, 33])
def test_regime_mixed(trx, orc, worlds, k):
    world = worlds(SC.CASES[0])
    surf, _, n, _ = _normals(trx, orc, world, k)
    differ = SC.differing(n, world[3]["attr"]["normal"][surf]).size / surf.size
    assert 0.01 <= differ <= 0.99, (k, differ)


def test_what_the_consumers_of_a_lost_normal_write(trx, orc, worlds):
    """What include/trx.h says of the normal's consumers beyond its range, on the twin (tests/test_gpu_scale.py holds the device to
    the twin at the same exponents).  k = +48, every normal all-zero: no facing test passes - every light, bounce-light and
    emitter ray is the inert ray, the light term is its ambient part alone, wgeo is +0 - and no neighbour passes the filters'
    normal test: the AO filter's term is the pixel's own count; the AO ray is still cast, along a finite direction.  k = -50,
    every normal has an infinite component: the AO ray's direction is NaN, point, rect and emitter lights still give +0 (their g
    and wgeo are NaN), and a directional light gives +inf at the few pixels whose normal is infinite without a NaN component (the ambient part alone elsewhere)."""
    world = worlds(SC.CASES[0])
    for k in (48, -50):
        s, p, f = _at(trx, orc, world, k)
        out = ST.twin_outputs(orc, s, p, f)
        surf = LT.surface(f.prim)
        syn = ST.synthetic(s, f.prim)
        assert (out["ao_rays"]["tmax"][surf] == np.float32(p.ao_radius)).all() and np.isfinite(out["ao_rays"]["origin"][surf]).all()
        assert (out["light_term_local"]["term"] == 0).all() and (out["emitter_wgeo"]["wgeo"] == 0).all() and (out["emitter_rays"]["tmax"] == -1).all()
        assert (out["light_rays_point"]["tmax"] == -1).all() and (out["light_rays_rect0"]["tmax"] == -1).all()
        directional = out["light_term_directional"]["term"][surf]
        if k == 48:
            for name in out:
                if "rays" in name and name != "ao_rays":
                    assert (out[name]["tmax"] == -1).all() and (out[name]["origin"] == 0).all(), name
            assert np.isfinite(out["ao_rays"]["direction"][surf]).all() and (directional == np.float32(0.25)).all()
            assert (out["bounce_weight_point"]["g"] == 0).all() and (out["bounce_weight_directional"]["g"] == 0).all()
            term = out["ao_filter"]["term"][surf]
            assert (term["samples"] == ST.AO_SAMPLES).all() and (term["unoccluded"] == syn.counts[surf]).all()
        else:
            assert np.isnan(out["ao_rays"]["direction"][surf]).any(1).all()
            assert np.isin(directional, [np.float32(0.25), np.float32(np.inf)]).all() and np.isposinf(directional).any()


# ---- the documented table ----------------------------------------------------------------------------------------------------------

def test_design_md_quotes_the_computed_table(trx, orc, worlds):
    """DESIGN.md's "scene scale" table is this tree's: every row ST.table_rows computes for the Cornell case stands in it."""
    world = worlds(SC.CASES[0])
    rows = ST.table_rows(trx, orc, world[0], world[1], world[2], world[3])
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    missing = [r for r in rows if r not in text]
    assert not missing, "DESIGN.md does not quote the computed table; the rows are:\n" + "\n".join(rows)
