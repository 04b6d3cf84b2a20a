"""The BVH refit's rule (include/trx.h, "refit") restated in numpy without a call into the library, and a checker of what
any correct refit must satisfy that shares none of the restatement's arithmetic.

refit(...) follows the header's words with np.float32 scalars, one node at a time, bottom-up:
  triangle box   first-of-equals min / max over v0, v1, v2
  leaf slot      the fold of its triangles' boxes in record order
  TLAS leaf      primitive k's box is the box of node instance_offsets[k] + entry[k]; with transforms its eight corners go
                 through ((m0 x + m4 y) + m8 z) + m12 per row and the result is padded by 1e-5 (max|.| + extent) + 1e-30
  node box       the fold over the non-empty slots 0..7
  origin         the box minimum, a zero as +0
  step           the power of two >= max(extent, 1e-20) / 255 read off the bits, doubled while ceil(extent / e) > 255 in
                 binary64; an extent of +inf starts at 1
  planes         f32 floor / ceil of (c - p) * (1 / e), clamped to 0..255, then corrected in binary64 until conservative
  kept           imask, both bases, child_meta, the bytes of empty slots, a node without children
Every min and max is `b if b < a else a`: which of +0 and -0 a minimum keeps is part of the rule, and numpy's minimum
does not promise one.

check_invariants(...) works in fractions.Fraction over the decoded bytes and the vertices: the topology is kept, every
decoded child box contains its exact content, every step is as small as the rule allows, every plane lies within two
steps of what it bounds."""
from fractions import Fraction

import numpy as np

F = np.float32
_INF = F(np.inf)
_FLT_MAX = F(3.402823466e+38)


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def _from_bits(u):
    return np.array(u, dtype=np.uint32).view(np.float32)[()]


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if a < b else a


def _leaf_count(m):
    return {1: 1, 3: 2, 7: 3}.get(m >> 5, 0)


def _is_inner(m):
    return (m & 0x18) == 0x18


def _segments(n_nodes, inst, tlas_start):
    """First node of every node's BVH segment (its child_base_idx is relative to it): the BLAS it lies in, or the TLAS."""
    seg = np.zeros(n_nodes, dtype=np.int64)
    if inst.size:
        starts = np.unique(inst.astype(np.int64))
        idx = np.searchsorted(starts, np.arange(n_nodes), side="right") - 1
        seg = np.where(idx >= 0, starts[np.maximum(idx, 0)], 0)
        seg[tlas_start:] = tlas_start
    return seg


def _dependencies(nodes, inst, entry, tlas_start):
    """Per node: [(slot, kind, ids)], kind "inner" (ids = [child node]), "tris" (ids = triangle records) or "inst" (ids =
    TLAS primitives)."""
    n = nodes.shape[0]
    b = nodes.view(np.uint8).reshape(n, 80)
    seg = _segments(n, inst, tlas_start)
    out = []
    for i in range(n):
        child_base, prim_base = int(nodes[i, 4]), int(nodes[i, 5])
        in_tlas = inst.size > 0 and i >= tlas_start
        rank, slots = 0, []
        for s in range(8):
            m = int(b[i, 24 + s])
            if m == 0:
                continue
            if _is_inner(m):
                slots.append((s, "inner", [int(seg[i]) + child_base + rank]))
                rank += 1
            else:
                first = prim_base + (m & 0x1f)
                slots.append((s, "inst" if in_tlas else "tris", list(range(first, first + _leaf_count(m)))))
        out.append(slots)
    return out


def _entry_node(inst, entry, k):
    return int(inst[k]) + (int(entry[k]) if entry is not None else 0)


def _heights(deps, inst, entry):
    n = len(deps)
    height = [-1] * n
    for root in range(n):
        if height[root] >= 0:
            continue
        stack = [(root, False)]
        while stack:
            i, done = stack.pop()
            below = []
            for _, kind, ids in deps[i]:
                below += ids if kind == "inner" else [_entry_node(inst, entry, k) for k in ids] if kind == "inst" else []
            if done:
                height[i] = 1 + max((height[d] for d in below), default=-1)
            elif height[i] < 0:
                assert len(stack) < 4 * n + 8, "the node references form a cycle"
                stack.append((i, True))
                stack += [(d, False) for d in below if height[d] < 0]
    return height


def _step(mn, mx):
    extent = mx - mn
    x = (F(1e-20) if extent < F(1e-20) else extent) * (F(1.0) / F(255.0))
    xb = _bits(x)
    if (xb & 0x7f800000) == 0x7f800000:
        e = F(1.0)
    else:
        e = _from_bits((((xb >> 23) + 1) << 23) if (xb & 0x7fffff) else xb)
    wide = float(mx) - float(mn)
    while np.ceil(wide / float(e)) > 255.0:
        e = e * F(2.0)
    return e


def _planes(p, e, cmn, cmx):
    rcp = F(1.0) / e
    lo = np.floor((cmn - p) * rcp)
    hi = np.ceil((cmx - p) * rcp)
    lo = F(0.0) if lo < F(0.0) else lo
    lo = F(255.0) if F(255.0) < lo else lo
    hi = F(0.0) if hi < F(0.0) else hi
    hi = F(255.0) if F(255.0) < hi else hi
    pd, ed = float(p), float(e)
    while lo > F(0.0) and pd + float(lo) * ed > float(cmn):
        lo = lo - F(1.0)
    while hi < F(255.0) and pd + float(hi) * ed < float(cmx):
        hi = hi + F(1.0)
    return int(lo) & 0xff, int(hi) & 0xff


def _world_box(mn, mx, m):
    wmn, wmx = [_FLT_MAX] * 3, [-_FLT_MAX] * 3
    for c in range(8):
        p = [mx[0] if c & 1 else mn[0], mx[1] if c & 2 else mn[1], mx[2] if c & 4 else mn[2]]
        for r in range(3):
            q = ((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r]
            wmn[r], wmx[r] = _min(wmn[r], q), _max(wmx[r], q)
    for a in range(3):
        pad = F(1e-5) * (_max(abs(wmn[a]), abs(wmx[a])) + (wmx[a] - wmn[a])) + F(1e-30)
        wmn[a], wmx[a] = wmn[a] - pad, wmx[a] + pad
    return wmn, wmx


def refit(nodes, tri_verts, instance_offsets=None, tlas_start=0, entry=None, object_to_world=None):
    """(new node buffer [n, 20] u32, per-node f32 boxes [n, 6], level sizes by height)."""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20)
    v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 3, 3)
    inst = np.ascontiguousarray(instance_offsets if instance_offsets is not None else [], dtype=np.uint32)
    entry = None if entry is None else np.ascontiguousarray(entry, dtype=np.uint32)
    o2w = None if object_to_world is None else np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 16)
    n = nodes.shape[0]
    out = nodes.copy()
    ob = out.view(np.uint8).reshape(n, 80)
    boxes = np.zeros((n, 6), dtype=np.float32)
    # triangle boxes: min(v0, min(v1, v2)), first of equals
    lt = lambda a, b: np.where(b < a, b, a)
    gt = lambda a, b: np.where(a < b, b, a)
    tmn = lt(v[:, 0], lt(v[:, 1], v[:, 2]))
    tmx = gt(v[:, 0], gt(v[:, 1], v[:, 2]))
    deps = _dependencies(nodes, inst, entry, int(tlas_start))
    height = _heights(deps, inst, entry)
    levels = np.bincount(np.asarray(height, dtype=np.int64)).tolist()
    with np.errstate(all="ignore"):
        for i in sorted(range(n), key=lambda k: (height[k], k)):
            nmn, nmx = [_INF] * 3, [-_INF] * 3
            child = {}
            for s, kind, ids in deps[i]:
                bmn, bmx = [_INF] * 3, [-_INF] * 3
                if kind == "inner":
                    bmn, bmx = list(boxes[ids[0], 0:3]), list(boxes[ids[0], 3:6])
                for j in ids if kind != "inner" else []:
                    if kind == "tris":
                        pmn, pmx = tmn[j], tmx[j]
                    else:
                        x = boxes[_entry_node(inst, entry, j)]
                        pmn, pmx = list(x[0:3]), list(x[3:6])
                        if o2w is not None:
                            pmn, pmx = _world_box(pmn, pmx, o2w[j])
                    for a in range(3):
                        bmn[a], bmx[a] = _min(bmn[a], pmn[a]), _max(bmx[a], pmx[a])
                child[s] = (bmn, bmx)
                for a in range(3):
                    nmn[a], nmx[a] = _min(nmn[a], bmn[a]), _max(nmx[a], bmx[a])
            if not child:   # the empty scene's root: left as it is, the point box at its origin
                boxes[i, 0:3] = boxes[i, 3:6] = nodes[i, 0:3].view(np.float32)
                continue
            for a in range(3):
                p = F(0.0) if nmn[a] == F(0.0) else nmn[a]
                e = _step(nmn[a], nmx[a])
                out[i, a] = _bits(p)
                ob[i, 12 + a] = (_bits(e) >> 23) & 0xff
                for s, (bmn, bmx) in child.items():
                    ob[i, 32 + 16 * a + s], ob[i, 40 + 16 * a + s] = _planes(p, e, bmn[a], bmx[a])
            boxes[i, 0:3], boxes[i, 3:6] = nmn, nmx
    return out, boxes, levels


# ---- invariants, in exact arithmetic -----------------------------------------------------------------------------------

EMPTY_META = 0


def _topology_kept(old, new):
    """imask, child_base_idx, primitive_base_idx, child_meta and the bytes of empty slots are the build's."""
    old = np.ascontiguousarray(old, dtype=np.uint32).reshape(-1, 20)
    new = np.ascontiguousarray(new, dtype=np.uint32).reshape(-1, 20)
    assert np.array_equal(old[:, 3] >> 24, new[:, 3] >> 24)          # imask
    assert np.array_equal(old[:, 4:8], new[:, 4:8])                   # bases + child_meta
    ob, nb = old.view(np.uint8).reshape(-1, 80), new.view(np.uint8).reshape(-1, 80)
    meta = ob[:, 24:32]
    for plane in range(6):                                            # min_x, max_x, min_y, max_y, min_z, max_z
        q = slice(32 + 8 * plane, 40 + 8 * plane)
        empty = meta == EMPTY_META
        assert np.array_equal(ob[:, q][empty], nb[:, q][empty])


def _fr(x):
    return Fraction(float(x))


def _exact_world(mn, mx, m):
    """(content, allowance) of a transformed box: the exact box of its eight corners through m, and how far beyond it the
    rule's f32 box may reach - its pad 1e-5 (max|.| + extent) + 1e-30 and the f32 rounding of the corner sums, each no more
    than a few 2^-24 of the sum of the terms' magnitudes S >= max|.|: together under 2e-5 (S + extent) + 2e-30."""
    m = [_fr(x) for x in m]
    lo, hi, mag = [None] * 3, [None] * 3, [Fraction(0)] * 3
    for c in range(8):
        p = [mx[0] if c & 1 else mn[0], mx[1] if c & 2 else mn[1], mx[2] if c & 4 else mn[2]]
        for r in range(3):
            terms = [m[r] * p[0], m[4 + r] * p[1], m[8 + r] * p[2], m[12 + r]]
            q = sum(terms)
            lo[r] = q if lo[r] is None or q < lo[r] else lo[r]
            hi[r] = q if hi[r] is None or q > hi[r] else hi[r]
            mag[r] = max(mag[r], sum(abs(t) for t in terms))
    allow = [Fraction(2, 100000) * (mag[a] + (hi[a] - lo[a])) + Fraction(2, 10 ** 30) for a in range(3)]
    return lo, hi, allow


def check_invariants(old_nodes, new_nodes, tri_verts, instance_offsets=None, tlas_start=0, entry=None, object_to_world=None):
    """Asserts what a refit of `old_nodes` over `tri_verts` must satisfy, whatever arithmetic produced `new_nodes`."""
    _topology_kept(old_nodes, new_nodes)
    nodes = np.ascontiguousarray(new_nodes, dtype=np.uint32).reshape(-1, 20)
    n = nodes.shape[0]
    b = nodes.view(np.uint8).reshape(n, 80)
    v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)   # (exact)
    inst = np.ascontiguousarray(instance_offsets if instance_offsets is not None else [], dtype=np.uint32)
    entry = None if entry is None else np.ascontiguousarray(entry, dtype=np.uint32)
    o2w = None if object_to_world is None else np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 16)
    tmn, tmx = v.min(axis=1), v.max(axis=1)
    deps = _dependencies(nodes, inst, entry, int(tlas_start))
    height = _heights(deps, inst, entry)
    # per node: what it must contain (inner) and what it may at most reach (outer); they differ by the instance pads only
    inner, outer = [None] * n, [None] * n

    def union(boxes):
        return ([min(x[0][a] for x in boxes) for a in range(3)], [max(x[1][a] for x in boxes) for a in range(3)])

    for i in sorted(range(n), key=lambda k: (height[k], k)):
        if not deps[i]:
            continue
        slot_in, slot_out = {}, {}
        for s, kind, ids in deps[i]:
            if kind == "inner":
                assert inner[ids[0]] is not None, "node %d: inner child %d has no children" % (i, ids[0])
                slot_in[s], slot_out[s] = inner[ids[0]], outer[ids[0]]
            elif kind == "tris":
                box = union([([_fr(x) for x in tmn[j]], [_fr(x) for x in tmx[j]]) for j in ids])
                slot_in[s] = slot_out[s] = box
            else:
                ins, outs = [], []
                for k in ids:
                    bi, bo = inner[_entry_node(inst, entry, k)], outer[_entry_node(inst, entry, k)]
                    if o2w is None:
                        ins.append(bi)
                        outs.append(bo)
                    else:   # (a BLAS box is exact: bi == bo)
                        lo, hi, allow = _exact_world(bi[0], bi[1], o2w[k])
                        ins.append((lo, hi))
                        outs.append(([lo[a] - allow[a] for a in range(3)], [hi[a] + allow[a] for a in range(3)]))
                slot_in[s], slot_out[s] = union(ins), union(outs)
        inner[i], outer[i] = union(list(slot_in.values())), union(list(slot_out.values()))
        for a in range(3):
            what = "node %d axis %d" % (i, a)
            pw, eb = int(nodes[i, a]), int(b[i, 12 + a])
            assert pw != 0x80000000, what + ": the origin is -0"
            assert 1 <= eb <= 254, what + ": step exponent byte %d" % eb
            p, e = _fr(nodes[i, a:a + 1].view(np.float32)[0]), Fraction(2) ** (eb - 127)
            assert outer[i][0][a] <= p <= inner[i][0][a], what + ": origin off the box minimum"
            assert p + 255 * e >= inner[i][1][a], what + ": 255 steps do not reach the far plane"
            assert eb == 53 or 255 * (e / 4) < outer[i][1][a] - outer[i][0][a], what + ": the step is larger than it must be"
            for s in slot_in:
                lo, hi = p + int(b[i, 32 + 16 * a + s]) * e, p + int(b[i, 40 + 16 * a + s]) * e
                assert lo <= slot_in[s][0][a] and hi >= slot_in[s][1][a], "%s slot %d: the planes cut the content" % (what, s)
                assert b[i, 32 + 16 * a + s] == 0 or lo > slot_out[s][0][a] - 2 * e, "%s slot %d: loose lower plane" % (what, s)
                assert b[i, 40 + 16 * a + s] == 255 or hi < slot_out[s][1][a] + 2 * e, "%s slot %d: loose upper plane" % (what, s)


# ---- the cases the host tests (test_refit_twin.py) and the device tests (test_gpu_refit_twin.py) share -------------------

def target_names():
    import adversarial_scenes as A
    return list(A.FINITE) + ["denormal", "one_point", "all_negative_zero", "near_flt_max"]


def target_size(name):
    return 10096 if name == "axis_segments_4096" else 6000   # (the generator writes 4096 segments from n / 3 on)


def target_verts(name, n):
    """Object-order vertices [n, 9] of a refit target: every finite adversarial scene, and four more the builder tests
    have no use for."""
    import adversarial_scenes as A
    if name in A.FINITE:
        return A.FINITE[name](n)
    if name == "denormal":            # every coordinate below the smallest normal binary32 number
        return (A.soup(n, 21).astype(np.float64) * 1e-39).astype(np.float32)
    if name == "one_point":
        return np.tile(np.array([0.3, -1.7, 2.5], dtype=np.float32), (n, 3))
    if name == "all_negative_zero":
        return np.full((n, 9), -0.0, dtype=np.float32)
    assert name == "near_flt_max"     # every extent of the root overflows binary32
    s = A.soup(n, 22).astype(np.float64)
    return (s / np.abs(s).max() * 3.4e38).astype(np.float32)


_soup_trees = {}


def soup_tree(trx, n):
    """The tree every target is refitted into: built once per size over the well-behaved soup, never changed."""
    import adversarial_scenes as A
    if n not in _soup_trees:
        _soup_trees[n] = trx.flat_build(A.soup(n, 1), np.array([n], dtype=np.uint64))
    return _soup_trees[n]


_kitchens = {}


def kitchen_tlas(trx, rebraid):
    """kitchen --tlas at 6000 triangles, re-braided (the default) or not: built once each, never changed."""
    if rebraid not in _kitchens:
        import ctypes
        lib = trx.load()
        assert lib.trx_set_build_rebraid(ctypes.c_float(1.0 / 4096.0 if rebraid else 0.0)) == 0
        try:
            v, c = trx.gen_scene("kitchen", 6000, 1)
            _kitchens[rebraid] = trx.flat_build(v, c, use_tlas=True)
        finally:
            lib.trx_set_build_rebraid(ctypes.c_float(1.0 / 4096.0))
    return _kitchens[rebraid]


def instance_transform_sets(trx, flat):
    """name -> [n_instances, 16] object-to-world matrices for helpers.instanced_scene: its own, random ones, mirrored ones
    far from the origin (the pad is then much larger than the boxes), tiny scales."""
    from helpers import random_affine
    own = np.ascontiguousarray(flat.instance_transforms, dtype=np.float32).reshape(-1, 16)
    rng = np.random.default_rng(41)
    mirrored = own.copy()
    mirrored[:, 0:3] = -mirrored[:, 0:3]            # (column 0 negated: determinant < 0)
    mirrored[:, 12:15] += np.float32(1e6)
    return {"own": own,
            "random": np.stack([random_affine(rng, spread=12.0) for _ in range(own.shape[0])]),
            "mirrored_far": mirrored,
            "tiny_scale": np.stack([random_affine(rng, 1e-6, 1e-5) for _ in range(own.shape[0])])}


def jitter(verts, seed, scale=0.01):
    """`verts` with every coordinate moved by a normal deviate of `scale` times the scene's diagonal."""
    v = np.asarray(verts, dtype=np.float64)
    p = v.reshape(-1, 3)
    size = float(np.linalg.norm(p.max(0) - p.min(0))) if p.size else 1.0
    return (v + np.random.default_rng(seed).normal(scale=scale * max(size, 1e-3), size=v.shape)).astype(np.float32)


def twin_of(flat, verts, o2w=None, nodes=None):
    """refit() with a FlatScene's tables."""
    return refit(flat.nodes if nodes is None else nodes, verts, flat.instance_offsets, flat.tlas_start, flat.instance_entry, o2w)


def check_flat(flat, new_nodes, verts, o2w=None):
    check_invariants(flat.nodes, new_nodes, verts, flat.instance_offsets, flat.tlas_start, flat.instance_entry, o2w)
