"""The record table of the caller-record tests (include/trx.h, "CALLER RECORDS"), and what the rule says of every entry -
written out by hand, column by column, not computed from any code under test.

THE RULE.  A primary record is a surface record of a scene iff t < FLT_MAX and prim < n_tris; every other record is a miss.
On a scene with instance transforms an instance id >= n_instances selects no row (the object-space normal is used as it
is), exactly as 0xFFFFFFFF always did.

THE TABLE.  Every t of T_TABLE crossed with every prim of prim_table(n_tris) - and, on a two-level scene, with every
instance id of inst_table(n_instances).  0x55555556 and 0xAAAAAAAB are there because three times the value wraps 32 bits
to 2 and 1: an index multiplied in 32 bits would land inside the table.

THE CANONICAL RECORD of an entry is what the rule says it means, in words every pass understood before the rule was
stated: a miss is {+inf, 0xFFFFFFFF} beside the instance id 0xFFFFFFFF; a surface record keeps its t and prim, and its
instance id where that selects a row, 0xFFFFFFFF where it does not.  A pass over doctored records must give what it gives
over their canonical records, bit for bit."""
import numpy as np

INVALID = 0xFFFFFFFF
FLT_MAX = np.float32(3.4028234663852886e38)
OWN = "own"   # the t the pixel's own record holds (a hit's finite t, +inf for a miss)


def _f(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


# (t, is it below FLT_MAX?) - the second column by hand.  OWN: yes iff the pixel's own record is a hit.
T_TABLE = [(OWN, None), (np.float32(1.0), True), (np.float32(-1.0), True), (np.float32(0.0), True), (_f(0x7F7FFFFE), True),
           (FLT_MAX, False), (np.float32(np.inf), False), (np.float32(np.nan), False)]
assert _f(0x7F7FFFFE) < FLT_MAX and _f(0x7F7FFFFF) == FLT_MAX


def prim_table(n_tris, near=False):
    """(prim, is it inside the triangle table?) - the second column by hand.  near: only the ids at the table's end."""
    assert 1 < n_tris < 2 ** 31 - 1 and n_tris + 1 not in (0x55555556, 0xAAAAAAAB)
    table = [(0, True), (n_tris - 1, True), (n_tris, False), (n_tris + 1, False)]
    if not near:
        table += [(2 ** 31, False), (0x55555556, False), (0xAAAAAAAB, False), (0xFFFFFFFE, False)]
    return table + [(INVALID, False)]


def inst_table(n_inst, near=False):
    """(instance id, does it select a row?) - the second column by hand."""
    assert 1 < n_inst < 2 ** 31 - 1
    table = [(0, True), (n_inst - 1, True), (n_inst, False), (n_inst + 1, False)]
    if not near:
        table += [(2 ** 31, False), (0xFFFFFFFE, False)]
    return table + [(INVALID, False)]


def entries(n_tris, n_inst=0, near=False):
    """The table: [(t, t_ok, prim, prim_ok, inst, inst_ok)], the instance columns (0xFFFFFFFF, False) on a single-level scene."""
    insts = inst_table(n_inst, near) if n_inst else [(INVALID, False)]
    return [(t, t_ok, p, p_ok, i, i_ok) for t, t_ok in T_TABLE for p, p_ok in prim_table(n_tris, near) for i, i_ok in insts]


TILE = 64   # the first TILE pixels of pick_pixels' list are the whole tile: doctor() gives them misses only


def pick_pixels(w, h, n_entries, surface):
    """The pixels to doctor, in four groups: one whole 8x8 tile (the inner tile with the most surface pixels; doctor() leaves
    no surface record in it, so a wave has nothing usable); the first and the last pixel of the image; a pixel of a ragged
    edge tile where the size has one; single pixels scattered over the other tiles - as many as it takes to place every entry
    of the table once outside the tile.  Returns (pixel ids y * w + x, the tile's first; the tile's pixel ids)."""
    tx = (w + 7) // 8
    py, px = np.divmod(np.arange(w * h), w)
    tile = (py // 8) * tx + px // 8
    inner = [t for t in range(tx * ((h + 7) // 8)) if (t % tx) * 8 + 8 <= w and (t // tx) * 8 + 8 <= h and t not in (tile[0], tile[-1])]
    best = max(inner, key=lambda t: int(surface[tile == t].sum()))
    whole = np.flatnonzero(tile == best)
    ends = [0, w * h - 1]
    ragged = [(h // 2) * w + (w - 1)] if w % 8 else [(h - 1) * w + w // 2] if h % 8 else []
    taken = set(whole.tolist()) | set(ends) | set(ragged)
    rest = np.array([i for i in range(w * h) if i not in taken and tile[i] != best])
    need = max(n_entries - len(ends) - len(ragged), 24)
    # an odd step over the remaining pixels: both parities of x and of y, every tile column
    step = rest.size // need
    step = max(step - 1 + step % 2, 1)
    scattered = rest[::step][:need]
    assert scattered.size == need, "the image is too small for the table"
    return np.concatenate([whole, ends, ragged, scattered]).astype(np.int64), whole


def doctor(prim, inst, pixels, table):
    """(doctored records, doctored ids, canonical records, canonical ids, is the doctored pixel a surface record?) for
    whole-image records `prim` / ids `inst` (None on a scene without ids) in pixel order.  The first TILE pixels - the whole
    tile - get the table's MISS entries in turn (a t below FLT_MAX beside a prim outside the table, a prim inside it beside a
    t that is not below FLT_MAX, and both at once): not one surface record is left there.  The other pixels get the whole
    table in turn, again from the first when they outnumber it."""
    assert len(pixels) - TILE >= len(table), "%d pixels for %d entries" % (len(pixels) - TILE, len(table))
    # (the own t beside a prim inside the table is a miss only where the pixel's own record is one: not for the tile)
    misses = [e for e in table if not e[3] or e[1] is False]
    assert len(misses) >= 16 and any(e[3] for e in misses) and any(e[1] for e in misses)
    dp, cp = prim.copy(), prim.copy()
    di = None if inst is None else inst.copy()
    ci = None if inst is None else inst.copy()
    is_surface = np.zeros(len(pixels), dtype=bool)
    for k, i in enumerate(pixels):
        # (the tile: the misses in turn - evenly spread over their list where they outnumber the tile, so both kinds are there)
        m = k * len(misses) // TILE if len(misses) > TILE else k % len(misses)
        t, t_ok, p, p_ok, ii, i_ok = misses[m] if k < TILE else table[(k - TILE) % len(table)]
        if t is OWN:
            t = prim["t"][i]
            t_ok = bool(np.isfinite(t))       # (a record the library wrote: a hit's t is finite, a miss holds +inf)
        dp["t"][i], dp["prim"][i] = t, p
        if di is not None:
            di[i] = ii
        if t_ok and p_ok:
            is_surface[k] = True
            cp["t"][i], cp["prim"][i] = t, p
            if ci is not None:
                ci[i] = ii if i_ok else INVALID
        else:
            cp["t"][i], cp["prim"][i] = np.inf, INVALID
            if ci is not None:
                ci[i] = INVALID
    assert not is_surface[:TILE].any()
    return dp, di, cp, ci, is_surface
