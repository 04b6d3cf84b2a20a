"""What tests/test_textures.py and tests/test_gpu_textures.py share: the scenes, the material tables, and the texcoord tables
and texture sets put on them.  Nothing here calls the library under test."""
import numpy as np

import material_twin as MT
import texture_twin as TT
from shading_normal_cases import GOLDENS, golden, record_verts  # noqa: F401

SCENES = GOLDENS                       # cornell_64, soup_52x44, cornell_tlas_48, kitchen_tlas_f16_56x40
TABLES = ("standin", "random", "hostile")
N_MATERIALS = 7


def materials(n_tris):
    """A seeded table of N_MATERIALS materials; material 1 emits whatever the seed says."""
    mat, idx = MT.seeded_table(n_tris, N_MATERIALS, 11)
    mat[1, 3:] = (2.0, 1.0, 0.5)
    return mat, idx


def tables(kind, recs, seed=0):
    """(uvs [n, 6] f32, TexSet) of table `kind` for triangles given as device records."""
    n = recs.shape[0]
    if kind == "standin":
        return TT.standin_texcoords(record_verts(recs)), TT.standin_textures(N_MATERIALS)
    if kind == "random":
        return TT.random_uvs(n, 77 + seed), TT.random_textures(N_MATERIALS, 5 + seed)
    assert kind == "hostile"
    return TT.hostile_uvs(n, 99 + seed), TT.random_textures(N_MATERIALS, 6 + seed)
