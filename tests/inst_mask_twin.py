"""The twin of a masked trace: the same scene with every invisible instance pointed at an EMPTY BLAS.

A childless node (no inner children, no leaf triangles) is inserted at index tlas_start and the TLAS moves up by one
(TLAS child bases are relative to the TLAS start, BLAS ones to their BLAS start: nothing else changes).  Every invisible
instance enters the empty node (entry node 0) and finds nothing there.  The TLAS itself - boxes, order, primitive ids -
is untouched, so an unmodified walk over the twin visits the TLAS exactly as the masked walk does, and its answer is the
masked answer bit for bit, tie-breaking included.

The device validates a node buffer against the BLAS segments named by instance_offsets: a BLAS with no visible instance
left drops out of that list, and its nodes then look like a part of the neighbouring segment.  Device twins therefore
need a visible instance per BLAS (`device_twin_ok`); patterns that hide a whole BLAS go to the oracle twin only."""
import numpy as np

from helpers import encode_node


def visible(masks, ray_mask):
    return (np.asarray(masks, dtype=np.uint32) & np.uint32(ray_mask)) != 0


def twin_buffers(flat, vis):
    """(nodes, instance_offsets, tlas_start, instance_entry or None) of the twin for the visibility vector `vis`."""
    ts = int(flat.tlas_start)
    empty = encode_node((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), [None] * 8, 0, 0)
    nodes = np.concatenate([flat.nodes[:ts], empty[None, :], flat.nodes[ts:]]).astype(np.uint32)
    inst = np.array(flat.instance_offsets, dtype=np.uint32)
    inst[~vis] = ts
    entry = getattr(flat, "instance_entry", None)
    if entry is not None:
        entry = np.array(entry, dtype=np.uint32)
        entry[~vis] = 0
    return nodes, inst, ts + 1, entry


def oracle_twin(orc, flat, vis, w2o=None):
    nodes, inst, ts, entry = twin_buffers(flat, vis)
    return orc.Scene(nodes, flat.tri_verts, inst, ts, instance_w2o=w2o, instance_entry=entry)


def device_twin_ok(flat, vis):
    return set(int(x) for x in np.asarray(flat.instance_offsets)[vis]) == set(int(x) for x in flat.instance_offsets)


def device_twin_flat(T, flat, vis):
    nodes, inst, ts, entry = twin_buffers(flat, vis)
    return T.FlatScene(nodes, flat.tri_verts, inst, ts, flat.tri_source, flat.blas_tri_start,
                       instance_transforms=getattr(flat, "instance_transforms", None), instance_entry=entry)
