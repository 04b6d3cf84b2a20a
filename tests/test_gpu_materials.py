"""Materials and the colour passes on the GPU, bit for bit (include/trx.h, "materials"): trx_scene_set_materials' tables (round
trip, accounting, replacement under a queued pass, refusals), trx_trace_indirect_rgb_dev and its sparse form against the twin
(tests/material_twin.py) - fed the device's own primary records - trx_material_compose_dev and trx_shade_rgb_dev against the
twin, trx_render_image_colour against its composition, and the red and green walls' tint on the Cornell floor.  Whole buffers
are compared, guard bytes past the last plane included; no record is left out.

The cases are tests/test_gpu_ao_visibility.py's - cornell_64 (64 x 64, single level), cornell_tlas_48 (48 x 48, two-level),
instanced (72 x 48, fourteen transformed instances), soup_52x44 (neither a multiple of 8), cornell_64_pipe (the padded twin) - and
kitchen_56x40, built here: eight transformed instances of the kitchen stand-in's objects, 56 x 40.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C

import numpy as np
import pytest

import light_twin as LT
import material_twin as MT
from ao_visibility_twin import record_map
from helpers import instanced_scene, random_rays
from hit_attr_twin import tri_records
from inst_mask_twin import oracle_twin
from test_gpu_ao_visibility import Case, make_case
from test_gpu_light import EPS, FILL, _buf, _dev, _mixed, _sync, _torch, limit

pytestmark = pytest.mark.gpu
UNIT = 64 * (32 + 1) + 64 * (32 + 8 + 4 + 24 + 4 + 4)   # scratch bytes the cap counts per tile and sample (kernels.h, kBounceUnitBytes)
GUARD = 64
f32 = np.float32
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


class Col:
    """A Case of tests/test_gpu_ao_visibility.py with what the colour twin needs of it.  The twin's material-free part - per
    sample s_f, the bounce's surface and its prim - is kept per argument set: a table only enters MT.term_rgb."""

    def __init__(self, case):
        self.case, self.w, self.h = case, case.w, case.h
        self.recs = tri_records(case.osc.verts)
        self.n_tris = self.recs.shape[0]
        self.w2o = case.osc.w2o if case.transformed else None
        self.cache, self._samples = {}, {}

    def samples(self, prim, inst, lights, frame0, n, sem, hidden=None):
        key = (hash(prim.tobytes()), hash(inst.tobytes()), tuple(l.key() for l in lights), frame0, n, sem, hidden)
        if key not in self._samples:
            osc, shadow = self.case.osc, None
            if hidden:
                import types
                vis = np.ones(osc.inst.size, dtype=bool)
                vis[list(hidden)] = False
                flat = types.SimpleNamespace(nodes=osc.nodes, tri_verts=osc.verts, instance_offsets=osc.inst, tlas_start=int(osc.c.tlas_start))
                shadow = oracle_twin(self.case.orc, flat, vis, w2o=osc.w2o)
            keep = []
            unit = np.array([[1, 1, 1, 0, 0, 0]], dtype=np.float32)
            MT.indirect_rgb(self.case.orc, osc, self.case.oview, self.w, self.h, prim, inst, self.recs, self.w2o, lights, frame0, n, EPS, EPS, sem,
                            unit, np.zeros(self.n_tris, dtype=np.uint16), shadow_osc=shadow, cache=self.cache, keep=keep)
            self._samples[key] = keep
        return self._samples[key]

    def twin(self, prim, inst, lights, frame0, n, sem, table, hidden=None):
        return MT.term_rgb(self.samples(prim, inst, lights, frame0, n, sem, hidden), prim, table[0], table[1], self.n_tris)

    def device(self, d_prim, d_inst, lights, n, sem, shard, frame0=0, stream=0, mask=0, sc=None):
        """(the three planes and GUARD bytes past them as bytes, the same buffer as it was before the call)."""
        _, _, size = record_map(self.w, self.h, shard)
        before = np.full(3 * size * 4 + GUARD, FILL, dtype=np.uint8)
        d_out = _dev(before)
        _sync()
        sc = sc or self.case.sc
        with limit():
            sc.trace_indirect_rgb_dev(self.case.view, self.w, self.h, [l.product(self.case.trx) for l in lights], d_prim.data_ptr(), d_out.data_ptr(),
                                      n_samples=n, sem=sem, ray_mask=mask, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS,
                                      d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0, shard=(*shard, 0), stream=stream)
            _torch().cuda.synchronize()
            sc.check()
        return d_out.cpu().numpy(), before

    def expected(self, values, before, shard):
        pix, rec, size = record_map(self.w, self.h, shard)
        want = before.copy()
        planes = want[:3 * size * 4].view(np.uint32).reshape(3, size)
        for c in range(3):
            planes[c, rec] = values[c].view(np.uint32)[pix]
        return want


def _check(col, d_prim, d_inst, prim, inst, lights, n, sem, shard, table, what, frame0=0, stream=0, mask=0, hidden=None, sc=None):
    got, before = col.device(d_prim, d_inst, lights, n, sem, shard, frame0=frame0, stream=stream, mask=mask, sc=sc)
    values = col.twin(prim, inst, lights, frame0, n, sem, table, hidden=hidden)
    _same(got, col.expected(values, before, shard), what)
    return values


class KitchenCase(Case):
    """The transformed kitchen at 56 x 40: eight transformed instances of the kitchen stand-in's objects seen from a corner of
    their box (the `instanced` case's construction over another scene and another image size)."""

    def __init__(self, trx, orc):
        self.trx, self.orc, self.name = trx, orc, "kitchen_56x40"
        flat, _, world, _, _ = instanced_scene(trx, seed=5, n_instances=8, tris_per_object=4000, kind="kitchen", spread=1.0)
        self.sc = trx.Scene(flat)
        self.osc = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=self.sc.instance_world_to_object())
        lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
        self.w, self.h = 56, 40
        self.eye, self.extent = hi + 0.1 * (hi - lo), float(((hi - lo) ** 2).sum())
        self.view = trx.view_from_camera(self.eye.tolist(), (0.5 * (lo + hi)).tolist(), 80.0, self.w, self.h)
        self.oview = orc.view_from_bytes(bytes(self.view))
        self.radius, self.transformed, self.base = 1.6, True, None
        self._rays, self._unoccluded = {}, {}


TABLE_SIZES = {"kitchen_56x40": 3, "cornell_64": 7, "cornell_tlas_48": 65536, "instanced": 5, "soup_52x44": 1, "cornell_64_pipe": 7}


@pytest.fixture(scope="module")
def cases(trx, orc):
    made, cols, tables = {}, {}, {}

    def get(name):
        if name == "kitchen_56x40" and name not in made:
            made[name] = KitchenCase(trx, orc)
        case = make_case(trx, orc, made, name)
        if name not in cols:
            cols[name] = Col(case)
            if case.base is not None:           # (a padded twin shares its base case's twin answers)
                cols[name].cache, cols[name]._samples = get(case.base.name)[0].cache, get(case.base.name)[0]._samples
            tables[name] = MT.seeded_table(cols[name].n_tris, TABLE_SIZES[name], 11)
            dev_idx = np.zeros(case.sc.flat.tri_verts.shape[0], dtype=np.uint16)      # (a padded twin: its appended records get material 0)
            dev_idx[:cols[name].n_tris] = tables[name][1]
            case.sc.set_materials(tables[name][0], dev_idx)
        return cols[name], tables[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def soup(trx):
    """A generated scene of 333 triangles (odd) and its stand-in palette: for the tables' own tests."""
    verts, counts = trx.gen_scene("soup", 333, 1)
    flat = trx.flat_build(verts, counts)
    mats, idx = trx.standin_materials("soup", verts, counts)
    return flat, mats, idx[flat.tri_source]


# ---- the tables -------------------------------------------------------------------------------------------------------------------

def test_set_get_round_trip_and_accounting(trx, soup):
    flat, mats, idx = soup
    n_tris = flat.tri_verts.shape[0]
    assert n_tris % 2 == 1 and idx.size == n_tris
    sc = trx.Scene(flat)
    try:
        bare = sc.device_bytes
        with pytest.raises(trx.TrxError, match="no materials"):
            sc.get_materials()
        sc.set_materials(mats, idx)
        got_m, got_i = sc.get_materials()
        assert got_m.tobytes() == mats.tobytes() and (got_i == idx).all()
        assert sc.device_bytes == bare + mats.size * 24 + n_tris * 2
        for n_mat in (1, 65536):
            m, i = MT.seeded_table(n_tris, n_mat, 5)
            assert i[0] == 0 and i[-1] == n_mat - 1 and {0, n_mat - 1} <= set(i.tolist())
            sc.set_materials(m, i)
            got_m, got_i = sc.get_materials()
            assert MT.table(got_m).tobytes() == m.tobytes() and (got_i == i).all() and got_m.shape[0] == n_mat
            assert sc.device_bytes == bare + n_mat * 24 + n_tris * 2          # (the old tables went with the swap)
        # a refit keeps both tables
        sc.refit(flat.tri_verts)
        got_m, got_i = sc.get_materials()
        assert MT.table(got_m).tobytes() == m.tobytes() and (got_i == i).all()
    finally:
        sc.close()


def test_every_refusal_leaves_the_old_table_in_force(trx, cases):
    col, (mat, idx) = cases("cornell_64")
    sc, n_tris = col.case.sc, col.n_tris
    from tray_racing_amd import _lib
    lib = trx.load()
    with limit():
        d_prim, d_inst, prim, inst = col.case.primary(0)
    lights = _mixed(1)
    before, _ = col.device(d_prim, d_inst, lights, 3, 0, (0, 1, 0))

    def raw(m=mat, n_mat=None, i=idx, n=n_tris):
        return lib.trx_scene_set_materials(sc.handle, None if m is None else m.ctypes.data_as(C.c_void_p), m.shape[0] if n_mat is None else n_mat,
                                           None if i is None else i.ctypes.data_as(C.c_void_p), n)

    def doctored(col_, value):
        m = mat.copy()
        m[3, col_] = value
        return m
    big = idx.copy()
    big[n_tris // 2] = mat.shape[0]
    last = idx.copy()
    last[-1] = 0xFFFF
    for kw, msg in (({"n_mat": 0}, b"n_materials"), ({"n_mat": 65537}, b"n_materials"), ({"n": n_tris - 1}, b"n_tris"), ({"n": n_tris + 1}, b"n_tris"),
                    ({"n": 0}, b"n_tris"), ({"i": big}, b"material index"), ({"i": last}, b"material index"), ({"m": None, "n_mat": 7}, b"null"), ({"i": None}, b"null"),
                    ({"m": doctored(0, -0.5)}, b"albedo"), ({"m": doctored(2, float("nan"))}, b"albedo"), ({"m": doctored(1, float("inf"))}, b"albedo"),
                    ({"m": doctored(3, -1e-30)}, b"emission"), ({"m": doctored(5, float("inf"))}, b"emission"), ({"m": doctored(4, float("nan"))}, b"emission")):
        assert raw(**kw) == _lib.TRX_ERR_INVALID and msg in lib.trx_last_error(), kw
    got_m, got_i = sc.get_materials()
    assert MT.table(got_m).tobytes() == mat.tobytes() and (got_i == idx).all()
    after, _ = col.device(d_prim, d_inst, lights, 3, 0, (0, 1, 0))
    _same(after, before, "the pass after the refused calls")
    n = C.c_uint32(mat.shape[0] - 1)                       # (too little room; a wrong triangle count)
    out_m, out_i = np.zeros((mat.shape[0], 6), dtype=np.float32), np.zeros(n_tris, dtype=np.uint16)
    assert lib.trx_scene_get_materials(sc.handle, out_m.ctypes.data_as(C.c_void_p), C.byref(n), out_i.ctypes.data_as(C.c_void_p), n_tris) == _lib.TRX_ERR_INVALID
    n = C.c_uint32(mat.shape[0])
    assert lib.trx_scene_get_materials(sc.handle, out_m.ctypes.data_as(C.c_void_p), C.byref(n), out_i.ctypes.data_as(C.c_void_p), n_tris - 1) == _lib.TRX_ERR_INVALID
    assert not out_m.any() and not out_i.any()


def test_colour_calls_are_refused_without_materials(trx, soup):
    flat, _, _ = soup
    sc = trx.Scene(flat)
    try:
        eye, look, fov = trx.scene_camera("soup")
        w, h = 24, 16
        view = trx.view_from_camera(eye, look, fov, w, h)
        n = w * h
        d_prim, d_out, d_rgba = _buf(n * 8, 0), _buf(3 * n * 4 + GUARD), _buf(n * 4)
        light = [trx.light(trx.LIGHT_POINT, (0, 1, 0))]
        with limit():
            sc.trace_primary_dev(view, w, h, d_prim.data_ptr())
            _torch().cuda.synchronize()
        for call in (lambda: sc.trace_indirect_rgb_dev(view, w, h, light, d_prim.data_ptr(), d_out.data_ptr(), n_samples=2),
                     lambda: sc.trace_indirect_rgb_sparse_dev(view, w, h, 2, 1, light, d_prim.data_ptr(), d_out.data_ptr(), n_samples=2),
                     lambda: sc.material_compose_dev(d_prim.data_ptr(), d_out.data_ptr(), n, d_out.data_ptr()),
                     lambda: sc.render_image_colour(view, w, h, light, bounce_samples=2)):
            with pytest.raises(trx.TrxError, match="no materials") as e:
                call()
            assert e.value.code == -1
        _sync()
        assert (d_out.cpu().numpy() == FILL).all()
        with limit():                                           # (the shade needs no materials)
            sc.shade_rgb_dev(d_out.data_ptr(), n, d_rgba.data_ptr())
            _torch().cuda.synchronize()
        sc.check()
    finally:
        sc.close()


def test_replacing_the_table_under_a_queued_pass(trx, cases):
    """The pass enqueued on a busy stream, then at once a new table: the call waits for the pass, which sees the old table in
    full; the next pass sees the new one."""
    torch = _torch()
    col, (mat, idx) = cases("soup_52x44")
    case = col.case
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    lights = _mixed(3)
    new = MT.seeded_table(col.n_tris, 9, 3)
    old_want = col.twin(prim, inst, lights, 0, 4, 0, (mat, idx))
    new_want = col.twin(prim, inst, lights, 0, 4, 0, new)
    assert (old_want.view(np.uint32) != new_want.view(np.uint32)).sum() > 100
    s = torch.cuda.Stream()
    big = random_rays(trx, case.flat, 1024 * 1024, 72, zero_dirs=False)
    d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
    size = case.w * case.h
    before = np.full(3 * size * 4 + GUARD, FILL, dtype=np.uint8)
    d_out, d_col = _dev(before), _dev(before)
    E = np.random.default_rng(4).uniform(0.0, 1.0, size).astype(np.float32)
    d_E = _dev(E)
    _sync()
    try:
        with limit():
            with torch.cuda.stream(s):
                case.sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), stream=s.cuda_stream)
                case.sc.trace_indirect_rgb_dev(case.view, case.w, case.h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_out.data_ptr(), n_samples=4,
                                               bounce_eps=EPS, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr(), stream=s.cuda_stream)
                # ... and a compose behind it on the same stream: it reads the tables on an image slot of its own
                case.sc.material_compose_dev(d_prim.data_ptr(), d_E.data_ptr(), size, d_col.data_ptr(), d_indirect_rgb=d_out.data_ptr(), stream=s.cuda_stream)
            case.sc.set_materials(*new)
            s.synchronize()
        _same(d_out.cpu().numpy(), col.expected(old_want, before, (0, 1, 0)), "the queued pass: the old table")
        want_col = before.copy()
        want_col[:3 * size * 4] = MT.compose(prim, E, old_want, mat, idx, col.n_tris).reshape(-1).view(np.uint8)
        _same(d_col.cpu().numpy(), want_col, "the queued compose: the old table")
        assert (MT.compose(prim, E, old_want, new[0], new[1], col.n_tris) != MT.compose(prim, E, old_want, mat, idx, col.n_tris)).sum() > 100
        _check(col, d_prim, d_inst, prim, inst, lights, 4, 0, (0, 1, 0), new, "the next pass: the new table")
    finally:
        case.sc.set_materials(mat, idx)


# ---- trx_trace_indirect_rgb_dev -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48", "instanced", "soup_52x44"])
def test_planes_equal_the_twin(trx, orc, cases, name):
    """1 and 3 lights of mixed kinds; 1, 3 and 16 samples; image layout, shard (1, 3) in both layouts with the other shards'
    records and the bytes past the last plane untouched; a non-null stream; TRX_SEM_HLSL and TRX_SEM_CPU; a frame0 whose seeds
    wrap past 2^32."""
    torch = _torch()
    col, table = cases(name)
    case = col.case
    st = torch.cuda.Stream()
    for sem, shard, stream, runs in ((0, (0, 1, 0), 0, ((1, 1, 3), (3, 3, 3), (3, 16, 0xFFFFFFF8))), (3, (1, 3, 1), st.cuda_stream, ((3, 3, 3), (1, 1, 0xFFFFFFFF))),
                                     (0, (1, 3, 0), 0, ((3, 3, 3),))):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem, shard, stream)
        for n_lights, n, frame0 in runs:
            values = _check(col, d_prim, d_inst, prim, inst, _mixed(n_lights), n, sem, shard, table,
                            "%s sem %d shard %s %d lights n %d frame0 %#x" % (name, sem, shard, n_lights, n, frame0), frame0=frame0, stream=stream)
            if shard == (0, 1, 0) and n > 1:
                surf = LT.surface(prim)
                assert (values[:, ~surf] == 0).all() and (values[:, surf] > 0).mean() > 0.05 and np.unique(values).size > 20, (name, n_lights, n)
                if table[0].shape[0] > 1:
                    assert (values[0] != values[1]).any() and (values[1] != values[2]).any(), name      # (colour, not three grey planes)


def test_planes_equal_the_twin_on_the_transformed_kitchen(trx, orc, cases):
    """56 x 40, eight transformed instances: a point light at the camera and a directional one, 3 samples, both layouts."""
    col, table = cases("kitchen_56x40")
    case = col.case
    lights = [LT.Light(LT.POINT, case.eye.tolist(), intensity=case.extent), LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5)]
    for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem, shard)
        values = _check(col, d_prim, d_inst, prim, inst, lights, 3, sem, shard, table, "kitchen_56x40 sem %d shard %s" % (sem, shard))
        if shard == (0, 1, 0):
            surf = LT.surface(prim)
            assert surf.mean() > 0.05 and (values[:, surf] > 0).mean() > 0.05 and np.unique(values).size > 20


def test_masked_shadow_rays_and_unit_albedo_identity(trx, orc, cases):
    """cornell_tlas_48: a masked pass against the twin scene of the visible instances; and with every albedo 1 and no emission the
    three planes are trx_trace_indirect_dev's values with bounce_albedo 1 and no base, on the device, bit for bit."""
    col, table = cases("cornell_tlas_48")
    case = col.case
    lights = _mixed(3)
    unit = (np.array([[1, 1, 1, 0, 0, 0]], dtype=np.float32), np.zeros(col.n_tris, dtype=np.uint16))
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
            masks[LT.MASK_HIDES] = 0x11
            case.sc.set_instance_masks(masks)
            _check(col, d_prim, d_inst, prim, inst, lights, 3, sem, shard, table, "sem %d ray_mask 0" % sem)
            masked = _check(col, d_prim, d_inst, prim, inst, lights, 3, sem, shard, table, "sem %d ray_mask 0x0E" % sem, mask=0x0E, hidden=(LT.MASK_HIDES,))
            if shard[1] == 1:
                assert (masked.view(np.uint32) != col.twin(prim, inst, lights, 0, 3, sem, table).view(np.uint32)).sum() > 10
            case.sc.set_instance_masks(None)
            case.sc.set_materials(*unit)
            got, before = col.device(d_prim, d_inst, lights, 3, sem, shard)
            _, _, size = record_map(col.w, col.h, shard)
            d_grey = _buf(size * 4)
            _sync()
            with limit():
                case.sc.trace_indirect_dev(case.view, col.w, col.h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_grey.data_ptr(), n_samples=3,
                                           sem=sem, bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=1.0, d_primary_inst=d_inst.data_ptr(), shard=(*shard, 0))
                _torch().cuda.synchronize()
            grey = d_grey.cpu().numpy()
            _same(got, np.concatenate([grey, grey, grey, before[3 * size * 4:]]), "unit albedo against the grey pass, sem %d shard %s" % (sem, shard))
            case.sc.set_materials(*table)
    finally:
        case.sc.set_instance_masks(None)
        case.sc.set_materials(*table)


@pytest.mark.parametrize("name", ["cornell_64", "instanced"])
def test_chunk_loops_give_the_same_planes(trx, orc, cases, name):
    """A scratch cap below the pass's need: samples in several chunks (three running sums added to), tiles in several chunks,
    both - bit for bit the twin's values, which know no chunking."""
    lib = trx.load()
    col, table = cases(name)
    case = col.case
    tiles = ((case.w + 7) // 8) * ((case.h + 7) // 8)
    lights, n = _mixed(3), 5
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (0, 1, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            for cap in (UNIT * tiles * 2, UNIT * tiles, UNIT * 10, UNIT * (tiles // 2 + 1) * 2, 1):
                lib.trx_debug_ao_scratch_cap(cap)
                _check(col, d_prim, d_inst, prim, inst, lights, n, sem, shard, table, "%s sem %d cap %d" % (name, sem, cap))
            lib.trx_debug_ao_scratch_cap(0)
    finally:
        lib.trx_debug_ao_scratch_cap(0)


def test_the_pipelined_walk_gives_the_same_planes(trx, orc, cases):
    col, table = cases("cornell_64_pipe")
    case = col.case
    assert case.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    _check(col, d_prim, d_inst, prim, inst, _mixed(3), 3, 0, (0, 1, 0), table, "pipelined", frame0=2)


# ---- trx_trace_indirect_rgb_sparse_dev -------------------------------------------------------------------------------------------

def _sparse(col, d_prim, d_inst, lights, n, stride, phase, frame0=0):
    wlo, hlo = (col.w + stride - 1) // stride, (col.h + stride - 1) // stride
    before = np.full(3 * wlo * hlo * 4 + GUARD, FILL, dtype=np.uint8)
    d_out = _dev(before)
    _sync()
    with limit():
        col.case.sc.trace_indirect_rgb_sparse_dev(col.case.view, col.w, col.h, stride, phase, [l.product(col.case.trx) for l in lights], d_prim.data_ptr(),
                                                  d_out.data_ptr(), n_samples=n, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS,
                                                  d_primary_inst=d_inst.data_ptr())
        _torch().cuda.synchronize()
        col.case.sc.check()
    return d_out.cpu().numpy(), before


def test_sparse_cells_are_the_dense_values_of_their_pixels(trx, orc, cases):
    """soup 52 x 44 (neither a multiple of 8, cells leave the image at strides 3 and 4): every phase at stride 2, one each at 3 and
    4; stride 1 is the dense pass."""
    col, table = cases("soup_52x44")
    with limit():
        d_prim, d_inst, prim, inst = col.case.primary(0)
    lights, n = _mixed(3), 3
    dense = col.twin(prim, inst, lights, 1, n, 0, table)
    left = 0
    for stride, phase in ((2, 0), (2, 1), (2, 2), (2, 3), (3, 7), (4, 15), (1, 0)):
        got, before = _sparse(col, d_prim, d_inst, lights, n, stride, phase, frame0=1)
        want = before.copy()
        lo = MT.sparse_rgb(dense, col.w, col.h, stride, phase)
        want[:lo.size * 4] = lo.reshape(-1).view(np.uint8)
        _same(got, want, "stride %d phase %d" % (stride, phase))
        left += int((((np.arange(lo.shape[1]) % ((col.w + stride - 1) // stride)) * stride + phase % stride) >= col.w).sum())
    assert left > 0                                                        # (cells whose pixel leaves the image: +0)
    one, _ = _sparse(col, d_prim, d_inst, lights, n, 1, 0, frame0=1)
    full, _ = col.device(d_prim, d_inst, lights, n, 0, (0, 1, 0), frame0=1)
    _same(one, full, "stride 1 against the dense pass")


# ---- compose and shade -----------------------------------------------------------------------------------------------------------

def test_compose_and_shade_equal_the_twin(trx, cases):
    """The device's own records in shard layout, then doctored caller records - prim at n_tris, far past it, 0xFFFFFFFF,
    t = FLT_MAX, a sentinel-filled tail - which must be background; with and without the indirect planes, aliased output; values
    at every code threshold and its lower neighbour, negative, NaN, +inf and exactly 1.0 through the shade."""
    torch = _torch()
    col, (mat, idx) = cases("cornell_64")
    sc, n_tris = col.case.sc, col.n_tris
    with limit():
        d_prim, _, _, _ = col.case.primary(0, (1, 3, 1))
    rec = d_prim.cpu().numpy().view(HIT).copy()
    n = rec.size
    rng = np.random.default_rng(n)
    hit = np.flatnonzero(rec["t"] < LT.F32_MAX)
    assert hit.size > 200
    rec["prim"][hit[0::9]] = n_tris
    rec["prim"][hit[1::9]] = n_tris + 12345678
    rec["prim"][hit[2::9]] = 0xFFFFFFFF
    rec["t"][hit[3::9]] = LT.F32_MAX
    rec.view(np.uint32)[-40:] = 0xA5A5A5A5                                  # (a sentinel-filled frame's records)
    thr = trx.image_code_table()
    E = rng.uniform(0.0, 1.2, n).astype(np.float32)
    I = rng.uniform(0.0, 0.8, (3, n)).astype(np.float32)
    special = np.concatenate([thr, np.nextafter(thr, f32(-1.0)), [f32(-1.0), f32("nan"), f32("inf"), f32(1.0), f32(-0.0)]]).astype(np.float32)
    d_rec, d_E = _dev(rec), _dev(E)
    for ind, alias in ((None, False), (I, False), (I, True)):
        before = np.full(3 * n * 4 + GUARD, FILL, dtype=np.uint8)
        if alias:
            before[:3 * n * 4] = I.reshape(-1).view(np.uint8)
        d_out = _dev(before)
        d_I = None if ind is None or alias else _dev(ind)
        _sync()
        with limit():
            sc.material_compose_dev(d_rec.data_ptr(), d_E.data_ptr(), n, d_out.data_ptr(),
                                    d_indirect_rgb=0 if ind is None else d_out.data_ptr() if alias else d_I.data_ptr())
            torch.cuda.synchronize()
        colour = MT.compose(rec, E, ind, mat, idx, n_tris)
        want = before.copy()
        want[:3 * n * 4] = colour.reshape(-1).view(np.uint8)
        _same(d_out.cpu().numpy(), want, "compose indirect %s alias %s" % (ind is not None, alias))
        surf = LT.surface(rec, n_tris)
        assert (colour[:, ~surf].view(np.uint32) == 0).all() and (colour[:, surf] > 0).any() and (~surf[hit[0::9]]).all() and (~surf[-5:]).all()
    # the shade: the composed colour with the special values spliced in
    colour = colour.copy()
    colour[0, :special.size], colour[1, -special.size:], colour[2, 100:100 + special.size] = special, special, special[::-1]
    before = np.full(n * 4 + GUARD, FILL, dtype=np.uint8)
    d_rgba, d_col = _dev(before), _dev(colour)
    _sync()
    with limit():
        sc.shade_rgb_dev(d_col.data_ptr(), n, d_rgba.data_ptr())
        torch.cuda.synchronize()
    want = before.copy()
    want[:n * 4] = MT.shade_rgb(colour, thr).reshape(-1)
    _same(d_rgba.cpu().numpy(), want, "the RGB shade")
    sc.check()


# ---- trx_render_image_colour -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bn,stride,levels,ao", [(0, 1, 0, 0), (3, 1, 0, 4), (3, 1, 2, 0), (3, 2, 3, 0), (2, 3, 0, 0)])
def test_host_form_is_its_composition(trx, cases, bn, stride, levels, ao):
    """Direct only, dense, dense + filter, sparse + upsample + filter, sparse + upsample: trx_render_image_colour against the
    device-resident calls it is made of, on the transformed scene."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    col, _ = cases("instanced")
    case = col.case
    sc, view, w, h = case.sc, case.view, case.w, case.h
    n = w * h
    lights, ls, sem, phase, up = _mixed(3), 4, 3, stride * stride - 1, 1
    products = [l.product(trx) for l in lights]
    with limit():
        img, ms = sc.render_image_colour(view, w, h, products, bounce_samples=bn, bounce_stride=stride, bounce_phase=phase, bounce_upsample_radius=up,
                                         bounce_filter_levels=levels, bounce_eps=EPS, sem=sem, frame0=2, light_samples=ls, shadow_eps=EPS, ambient=0.3,
                                         ao_samples=ao, ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
    d_prim, d_inst, d_attr, d_lit = _buf(n * 8, 0xEE), _buf(n * 4, 0xFF), _buf(n * 24, 0), _buf(len(lights) * n)
    d_cnt, d_term, d_val, d_rgba = _buf(n), _buf(n * 4), _buf(n * 4), _buf(n * 4)
    d_a, d_b, d_work = _buf(3 * n * 4), _buf(3 * n * 4), _buf(n * 4)
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        sc.hit_attributes_primary_dev(view, w, h, d_prim.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
        sc.trace_light_visibility_dev(view, w, h, products, d_prim.data_ptr(), d_lit.data_ptr(), n_samples=ls, sem=sem, frame0=2, shadow_eps=EPS,
                                      d_primary_inst=d_inst.data_ptr())
        if ao:
            sc.trace_ao_visibility_dev(view, w, h, d_prim.data_ptr(), d_cnt.data_ptr(), ao, case.radius, sem=sem, frame0=2, ao_eps=EPS,
                                       d_primary_inst=d_inst.data_ptr())
            sc.ao_filter_dev(w, h, d_prim.data_ptr(), d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=d_attr.data_ptr())
        sc.light_term_dev(view, w, h, products, d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(), n_samples=ls, ambient=0.3,
                          d_term=d_term.data_ptr() if ao else 0)
        planes = 0
        if bn:
            planes, other = d_a.data_ptr(), d_b.data_ptr()
            if stride > 1:
                sc.trace_indirect_rgb_sparse_dev(view, w, h, stride, phase, products, d_prim.data_ptr(), planes, n_samples=bn, sem=sem, frame0=2,
                                                 bounce_eps=EPS, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                n_lo = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
                for c in range(3):
                    sc.value_upsample_dev(w, h, stride, phase, d_prim.data_ptr(), planes + c * n_lo * 4, other + c * n * 4, up, d_attr=d_attr.data_ptr())
                planes, other = other, planes
            else:
                sc.trace_indirect_rgb_dev(view, w, h, products, d_prim.data_ptr(), planes, n_samples=bn, sem=sem, frame0=2, bounce_eps=EPS,
                                          shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
            if levels:
                for c in range(3):
                    sc.value_filter_dev(w, h, d_prim.data_ptr(), planes + c * n * 4, other + c * n * 4, levels, d_attr=d_attr.data_ptr(),
                                        d_work=d_work.data_ptr())
                planes, other = other, planes
        colour = planes or d_a.data_ptr()
        sc.material_compose_dev(d_prim.data_ptr(), d_val.data_ptr(), n, colour, d_indirect_rgb=planes)
        sc.shade_rgb_dev(colour, n, d_rgba.data_ptr())
        torch.cuda.synchronize()
    want = d_rgba.cpu().numpy().reshape(h, w, 4)
    assert ms > 0 and (img == want).all(), (bn, stride, levels, (img != want).sum())
    assert (img[..., 3] == 255).all() and (img[..., 0] != img[..., 1]).mean() > 0.02      # (a colour image)
    sc.check()


# ---- the Cornell box: the walls tint the floor ------------------------------------------------------------------------------------

def test_the_cornell_walls_tint_the_floor_beside_them(trx, orc):
    """The stand-in Cornell box with its stand-in table (by tri_source), one point light, 16 bounce samples: on the twin the
    floor's column of triangles beside the red wall gathers more red than green, the column beside the green wall more green than
    red - and the device's planes are the twin's."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    table = (MT.table(mats), idx[flat.tri_source])
    want_m, want_i = MT.standin("cornell", verts, counts)
    assert (table[0] == want_m).all() and (table[1] == want_i[flat.tri_source]).all() and set(table[1].tolist()) == {0, 1, 2, 3}
    v = flat.tri_verts.reshape(-1, 3, 3)
    w = h = 64
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, w, h)
    sc = trx.Scene(flat)
    try:
        sc.set_materials(*table)
        osc = orc.Scene.from_flat(flat)
        recs = tri_records(flat.tri_verts)
        d_prim, d_out = _buf(w * h * 8, 0xEE), _buf(3 * w * h * 4 + GUARD)
        light = LT.Light(LT.POINT, (0.0, 1.8, 0.0), intensity=1.5)
        with limit():
            sc.trace_primary_dev(view, w, h, d_prim.data_ptr())
            sc.trace_indirect_rgb_dev(view, w, h, [light.product(trx)], d_prim.data_ptr(), d_out.data_ptr(), n_samples=16, bounce_eps=EPS, shadow_eps=EPS)
            _torch().cuda.synchronize()
            sc.check()
        prim = d_prim.cpu().numpy().view(orc.HIT_DTYPE)
        inst = np.full(w * h, 0xFFFFFFFF, dtype=np.uint32)
        twin = MT.indirect_rgb(orc, osc, orc.view_from_bytes(bytes(view)), w, h, prim, inst, recs, None, [light], 0, 16, EPS, EPS, 0, *table)
        floor = (v[:, :, 1] == 0.0).all(1) & (table[1] == 0)
        beside_red, beside_green = floor & (v[:, :, 0].min(1) == -1.0), floor & (v[:, :, 0].max(1) == 1.0)
        assert beside_red.sum() >= 12 and beside_green.sum() >= 12
        surf = LT.surface(prim)
        at = np.where(surf, prim["prim"], 0)
        px_red, px_green = surf & beside_red[at], surf & beside_green[at]
        assert px_red.sum() > 30 and px_green.sum() > 30
        assert twin[0][px_red].mean() > 1.05 * twin[1][px_red].mean() and (twin[0][px_red] >= twin[1][px_red]).mean() > 0.75
        assert twin[1][px_green].mean() > 1.05 * twin[0][px_green].mean() and (twin[1][px_green] >= twin[0][px_green]).mean() > 0.75
        want = np.full(3 * w * h * 4 + GUARD, FILL, dtype=np.uint8)
        want[:3 * w * h * 4] = twin.reshape(-1).view(np.uint8)
        _same(d_out.cpu().numpy(), want, "the Cornell box's planes")
    finally:
        sc.close()
