"""The packet test of a wave-uniform node step (kernels.hip node_intersect_kept, trace_walk_plain.inc) restated in numpy
float32 and checked as a PROPERTY: a child the packet test leaves out is missed by every ray of the packet.  The bounds
are the per-ray test's own multiplications and additions evaluated at the ends of the rays' 1/d interval; what makes them
bounds is that round-to-nearest products and sums are monotone in each operand - this test does not assume it, it looks.
Also the literal-division variants: b = RN(c / d) per ray against the interval of RN(c RN(1/d)) moved out by 2^-21."""
import numpy as np

F = np.float32


def per_ray_slabs(o, d, p, e, q_lo, q_hi, literal):
    """tmin / tmax of every (ray, child) as node_intersect computes them (query.hlsl:237-300), without the t clamp.
    o, d: [R, 3]; p: [3]; e: [3] (powers of two); q_lo, q_hi: [8, 3] bytes.  literal: b = (p - o) / d, else (p - o) * (1/d)."""
    ix = F(1.0) / d
    a = e[None, :] * ix
    c = p[None, :] - o
    b = (c / d) if literal else (c * ix)
    neg = d < 0
    qn = np.where(neg[:, None, :], q_hi[None], q_lo[None]).astype(F)   # near plane: the max plane where d < 0
    qf = np.where(neg[:, None, :], q_lo[None], q_hi[None]).astype(F)
    tn = qn * a[:, None, :] + b[:, None, :]
    tf = qf * a[:, None, :] + b[:, None, :]
    tmin = np.fmax(np.fmax(np.fmax(tn[:, :, 0], tn[:, :, 1]), tn[:, :, 2]), F(0.0001))
    tmax = np.fmin(np.fmin(tf[:, :, 0], tf[:, :, 1]), tf[:, :, 2])
    return tmin, tmax


def packet_keep(o, d, p, e, q_lo, q_hi, literal, guard=True):
    """The packet test: [8] bools, False = no ray of the packet can enter the child.  guard=False leaves the `finite`
    guard out: test_the_finite_guard_is_what_keeps_partly_overflowing_planes_from_culling shows what it is for."""
    ix = F(1.0) / d
    lo, hi = ix.min(axis=0), ix.max(axis=0)            # per axis; one sign per axis (the caller's packets share an octant)
    neg = lo < 0
    c = p - o[0]
    alo, ahi = e * lo, e * hi
    b0, b1 = c * lo, c * hi
    blo, bhi = np.fmin(b0, b1), np.fmax(b0, b1)
    if literal:
        blo = (blo - np.abs(blo) * F(2.0 ** -21)).astype(F)
        bhi = (bhi + np.abs(bhi) * F(2.0 ** -21)).astype(F)
    # per axis: all four products finite - fmaxf drops a NaN among them, so a NaN alone does not clear the flag
    finite = np.fmax(np.fmax(np.abs(alo), np.abs(ahi)), np.fmax(np.abs(b0), np.abs(b1))) < F(np.inf)
    qn = np.where(neg[None, :], q_hi, q_lo).astype(F)
    qf = np.where(neg[None, :], q_lo, q_hi).astype(F)
    lb = qn * alo[None, :] + blo[None, :]
    ub = qf * ahi[None, :] + bhi[None, :]
    if guard:
        lb = np.where(finite[None, :], lb, F(-np.inf))
        ub = np.where(finite[None, :], ub, F(np.inf))
    tmin_lb = np.fmax(np.fmax(np.fmax(lb[:, 0], lb[:, 1]), lb[:, 2]), F(0.0001))
    tmax_ub = np.fmin(np.fmin(ub[:, 0], ub[:, 1]), ub[:, 2])
    return ~(tmin_lb > tmax_ub)


def random_packet(rng, spread):
    """64 rays from one origin inside a narrow cone (an 8x8 tile), all in one octant, and a node frame in front of them."""
    o = np.tile(rng.uniform(-50, 50, 3).astype(F), (64, 1))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    d = (axis[None, :] + spread * rng.uniform(-1, 1, (64, 3))).astype(F)
    d[np.abs(d) < 1e-6] = F(1e-6)
    same = (np.sign(d) == np.sign(d[0])).all()
    e_exp = rng.integers(-8, 6, 3)
    e = (F(2.0) ** e_exp.astype(F)).astype(F)
    centre = o[0].astype(np.float64) + axis * rng.uniform(0.5, 400) + rng.normal(size=3) * rng.uniform(0, 60)
    p = (centre - 128.0 * e.astype(np.float64) * rng.uniform(0, 1.5, 3)).astype(F)
    q_lo = rng.integers(0, 250, (8, 3))
    q_hi = np.minimum(q_lo + rng.integers(0, 60, (8, 3)), 255)
    return same, o, d, p, e, q_lo.astype(np.uint8), q_hi.astype(np.uint8)


def test_a_child_the_packet_test_leaves_out_is_missed_by_every_ray():
    rng = np.random.default_rng(11)
    culled = kept = packets = 0
    for literal in (False, True):
        for k in range(4000):
            same, o, d, p, e, q_lo, q_hi = random_packet(rng, spread=rng.choice([0.002, 0.01, 0.05]))
            if not same:
                continue   # (the kernel does not run the packet test on a wave whose rays span octants)
            packets += 1
            tmin, tmax = per_ray_slabs(o, d, p, e, q_lo, q_hi, literal)
            keep = packet_keep(o, d, p, e, q_lo, q_hi, literal)
            enters = (tmin <= tmax).any(axis=0)          # per child: some ray enters it
            assert not (enters & ~keep).any(), (literal, k)
            culled += int((~keep).sum())
            kept += int(keep.sum())
    # ... and the test is worth running: it leaves out most children, and what it keeps is mostly entered by some ray
    assert packets > 6000 and culled > 2 * kept


def test_the_bounds_bound_plane_by_plane():
    """Finer than the mask: for every child and axis the packet's near bound is <= every ray's near parameter and its far
    bound >= every ray's far parameter."""
    rng = np.random.default_rng(12)
    for literal in (False, True):
        for k in range(1500):
            same, o, d, p, e, q_lo, q_hi = random_packet(rng, spread=0.02)
            if not same:
                continue
            ix = F(1.0) / d
            a = e[None, :] * ix
            c = p[None, :] - o
            b = (c / d) if literal else (c * ix)
            neg = d[0] < 0
            qn = np.where(neg[None, :], q_hi, q_lo).astype(F)
            qf = np.where(neg[None, :], q_lo, q_hi).astype(F)
            tn = qn[None] * a[:, None, :] + b[:, None, :]
            tf = qf[None] * a[:, None, :] + b[:, None, :]
            lo, hi = ix.min(axis=0), ix.max(axis=0)
            alo, ahi = e * lo, e * hi
            b0, b1 = c[0] * lo, c[0] * hi
            blo, bhi = np.minimum(b0, b1), np.maximum(b0, b1)
            if literal:
                blo = (blo - np.abs(blo) * F(2.0 ** -21)).astype(F)
                bhi = (bhi + np.abs(bhi) * F(2.0 ** -21)).astype(F)
            assert (qn * alo[None, :] + blo[None, :] <= tn.min(axis=0)).all(), (literal, k)
            assert (qf * ahi[None, :] + bhi[None, :] >= tf.max(axis=0)).all(), (literal, k)


def hostile_packet(rng):
    """A packet as the hostile cameras make them: one origin for 64 rays of one octant; on one axis the direction runs from
    the zero-direction fix (or a rounding residue beside zero) up to a pixel's width, so 1/d spans up to 1/eps; the node
    frame has c = p - o = +0 on an axis, exponent bytes up to 254 (e * ix overflows), and now and then a NaN origin
    component (the walk's origin test compares bit patterns, which a NaN passes)."""
    eps = F(1.1920929e-7)
    o = rng.uniform(-50, 50, 3).astype(F)
    sign = np.where(rng.integers(2, size=3) == 1, F(1), F(-1))
    d = (np.abs(rng.normal(size=(64, 3))) * 0.3 + 0.05).astype(F)
    k = int(rng.integers(3))
    d[:, k] = np.abs(rng.uniform(0, 1, 64) * rng.choice([1e-8, 1e-6, 1e-3, 0.1])).astype(F)
    d[: int(rng.integers(1, 9)), k] = F(0.0)
    d[d == 0] = eps                                    # finish_ray_dir's fix: the octant counts a fixed zero as positive
    d[:, k] = np.where(d[:, k] == eps, eps, d[:, k] * sign[k])
    if (np.sign(d[:, k]) != np.sign(d[0, k])).any():   # a negative axis whose zeros were fixed to +eps spans two octants:
        d[:, k] = np.abs(d[:, k])                      # the walk would not run the packet test on it
    for a in range(3):
        if a != k:
            d[:, a] *= sign[a]
    e_byte = np.where(rng.integers(4, size=3) == 0, rng.integers(200, 255, 3), rng.integers(100, 140, 3))
    e = (e_byte.astype(np.uint32) << np.uint32(23)).view(F)
    p = (o.astype(np.float64) + rng.normal(size=3) * 40).astype(F)
    zero_c = rng.integers(3, size=3) == 0
    p[zero_c] = o[zero_c]                              # c = +0 on those axes
    if rng.integers(5) == 0:
        o[int(rng.integers(3))] = F(np.nan)
    q_lo = rng.integers(0, 250, (8, 3))
    q_hi = np.minimum(q_lo + rng.integers(0, 60, (8, 3)), 255)
    return np.tile(o, (64, 1)), d, p, e, q_lo.astype(np.uint8), q_hi.astype(np.uint8)


def test_hostile_packets_a_child_left_out_is_still_missed_by_every_ray():
    """The same property on the packets of hostile cameras, where products overflow, 0 x inf makes NaNs and a NaN origin
    component gets through: no child the packet test leaves out is entered by any ray under the per-ray test's own
    fmaxf / fminf.  The generator reaches what it is for (infinite products, NaN bounds, culled and kept children)."""
    rng = np.random.default_rng(21)
    culled = kept = nonfinite = nan_origin = wide = 0
    with np.errstate(all="ignore"):
        for literal in (False, True):
            for k in range(3000):
                o, d, p, e, q_lo, q_hi = hostile_packet(rng)
                tmin, tmax = per_ray_slabs(o, d, p, e, q_lo, q_hi, literal)
                keep = packet_keep(o, d, p, e, q_lo, q_hi, literal)
                enters = (tmin <= tmax).any(axis=0)
                assert not (enters & ~keep).any(), (literal, k)
                culled += int((~keep).sum())
                kept += int(keep.sum())
                ix = F(1.0) / d
                nonfinite += int(not np.isfinite(e[None, :] * ix).all())
                nan_origin += int(np.isnan(o).any())
                wide += int((np.abs(ix).max(axis=0) / np.abs(ix).min(axis=0)).max() > 1e5)
    assert culled > 1000 and kept > 1000 and nonfinite > 500 and nan_origin > 500 and wide > 500


def partly_overflowing_packet(rng):
    """What the `finite` guard is for, built on purpose: on axis k the rays' 1/d runs from about 10 to 1/eps = 2^23 and the
    node's exponent byte is so large that e * (1/d) overflows at the upper end of the interval only; every child's near
    plane on that axis is q = 0.  A ray at the upper end computes 0 x inf = NaN for that plane and its fmaxf drops it -
    the ray ignores the plane - while the packet's bound 0 x alo + blo is finite and, with the node ahead on that axis
    (c > 0), large.  On the other two axes the children straddle the origin, so such a ray does enter them."""
    eps = F(1.1920929e-7)
    k = int(rng.integers(3))
    o = rng.uniform(-50, 50, 3).astype(F)
    sign = np.where(rng.integers(2, size=3) == 1, F(1), F(-1))
    sign[k] = F(1)
    d = (rng.uniform(0.2, 0.9, (64, 3)) * sign[None, :]).astype(F)
    d[:, k] = (rng.uniform(0.02, 0.1, 64)).astype(F)
    d[: int(rng.integers(1, 9)), k] = eps                  # zero components after finish_ray_dir's fix
    e_byte = rng.integers(118, 126, 3)
    e_byte[k] = rng.integers(232, 241)                     # 2^105 .. 2^113: x 2^23 overflows, x 50 does not
    e = (e_byte.astype(np.uint32) << np.uint32(23)).view(F)
    p = (o.astype(np.float64) - 128.0 * e.astype(np.float64) * rng.uniform(0.5, 1.0, 3)).astype(F)
    p[k] = F(o[k] + rng.uniform(1.0, 1e4))
    q_lo = rng.integers(0, 100, (8, 3))
    q_hi = rng.integers(156, 256, (8, 3))
    q_lo[:, k] = 0
    return np.tile(o, (64, 1)), d, p, e, q_lo.astype(np.uint8), q_hi.astype(np.uint8)


def test_the_finite_guard_is_what_keeps_partly_overflowing_planes_from_culling():
    """With the guard the property holds on these packets; without it (packet_keep(guard=False): the walk with
    trace_walk_plain.inc's `if (!finite) bound = ...` line dropped) the packet test leaves out children that rays enter -
    so this restatement notices the guard going missing."""
    rng = np.random.default_rng(31)
    broken = entered = 0
    with np.errstate(all="ignore"):
        for literal in (False, True):
            for k in range(500):
                o, d, p, e, q_lo, q_hi = partly_overflowing_packet(rng)
                tmin, tmax = per_ray_slabs(o, d, p, e, q_lo, q_hi, literal)
                enters = (tmin <= tmax).any(axis=0)
                entered += int(enters.sum())
                assert not (enters & ~packet_keep(o, d, p, e, q_lo, q_hi, literal)).any(), (literal, k)
                broken += int((enters & ~packet_keep(o, d, p, e, q_lo, q_hi, literal, guard=False)).any())
    assert entered > 4000 and broken > 500, (entered, broken)
