"""What tests/test_shading_normals.py and tests/test_gpu_shading_normals.py share: the scenes, the vertex-normal tables set on
them, and the unit cube of the generator's tests.  Nothing here calls the library under test except to generate the transformed
two-level scene (ao_visibility_twin.instanced_case, as tests/test_gpu_light.py builds it)."""
import os

import numpy as np

import shading_normal_twin as SN
from hit_attr_twin import tri_records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("cornell_64", "soup_52x44", "cornell_tlas_48", "kitchen_tlas_f16_56x40")
SCENES = GOLDENS + ("instanced",)
TABLES = ("computed", "random", "hostile")
WELD_ALL = -1.0        # the crease of the "computed" table: every face at a corner is welded, so normals tilt across box edges


def record_verts(recs):
    """[n, 9] f32 vertices of device records {v0, e1 = v0 - v1, e2 = v2 - v0, ng}: what the kernels see of a triangle (the
    decoded vertices of a TRX_TRI_F16_24 scene)."""
    v0, e1, e2 = recs[:, 0:3], recs[:, 3:6], recs[:, 6:9]
    return np.concatenate([v0, v0 - e1, v0 + e2], axis=1).astype(np.float32)


def golden(name):
    """(fixture, records [n, 12], f16 words or None) of a golden scene."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    f16 = g["tri_f16"] if "tri_f16" in g.files else None
    return g, (tri_records(tri_f16=f16) if f16 is not None else tri_records(g["tri_verts"])), f16


def table(kind, recs, seed=0):
    """[n, 9] f32: the vertex-normal table `kind` for triangles given as device records."""
    if kind == "computed":
        return SN.vertex_normals(record_verts(recs), WELD_ALL)
    if kind == "random":
        rng = np.random.default_rng(1234 + seed)
        t = rng.normal(size=(recs.shape[0], 9)).astype(np.float32)
        t *= rng.choice(np.array([1e-3, 1.0, 1.0, 7.5, 1e4], dtype=np.float32), size=(recs.shape[0], 1))    # (unnormalised is legal)
        return t.astype(np.float32)
    assert kind == "hostile"
    return SN.hostile_normals(recs)


def cube():
    """[12, 9] f32: the unit cube, faces wound outward, every face split along the diagonal between its two corners of even
    coordinate sum - so a corner has either two triangles of each of its three faces or one of each."""
    tris = []
    for axis in range(3):
        for side in (0, 1):
            a, b = (axis + 1) % 3, (axis + 2) % 3

            def corner(i, j):
                p = [0.0, 0.0, 0.0]
                p[axis], p[a], p[b] = float(side), float(i), float(j)
                return p
            quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]          # counter-clockwise seen from +axis
            if side == 0:
                quad = quad[::-1]
            even = [k for k in range(4) if int(sum(quad[k])) % 2 == 0]
            assert len(even) == 2 and (even[1] - even[0]) == 2
            k0 = even[0]
            q = quad[k0:] + quad[:k0]                                                  # (the diagonal runs q[0] - q[2])
            tris += [q[0] + q[1] + q[2], q[0] + q[2] + q[3]]
    return np.array(tris, dtype=np.float32)
