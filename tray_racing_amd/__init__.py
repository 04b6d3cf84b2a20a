"""tray_racing_amd — MI355X (gfx950) backend for tray_racing's CWBVH traversal hot path.

`csrc/` holds the HIP kernels and the C-ABI (include/trx.h); `host.py` mirrors
the reference's `cwbvh_gpu_runner` / `rt_gpu_software::start` interface over it.
"""
from ._lib import (SEM_CPU, SEM_HLSL, SEM_NODE_FMA, SEM_NODE_RCP, SEM_TIE_FIRST, TRI_EDGES_36, TRI_F16_24,  # noqa: F401
                   TRI_VERTS_36, MODE_AO, MODE_FUSED, MODE_PRIMARY, MODE_RAYS, MODE_SERVICE, WALK_PIPELINED, WALK_PLAIN, HEAT_NODES, HEAT_SCALE_NODES, HEAT_SCALE_TRIS, HEAT_TRIS, LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_RECT, MAX_LIGHTS, MAX_MATERIALS, MAX_EMITTERS, AoTerm, Light, Material, Hit, HitAttr, Ray, RayCost, RayHit, Shard, Stats, TrxError, View, load)
from .host import (AO_TERM_DTYPE, HIT_ATTR_DTYPE, HIT_DTYPE, MISS_PRIM, RAY_COST_DTYPE, RAY_DTYPE, RAYHIT_DTYPE, MATERIAL_DTYPE, FlatScene, Scene, cwbvh_gpu_runner, flat_build, flat_build_instanced, flat_build_params, flat_build_preset_device, build_params, gen_scene,  # noqa: F401
                   image_code_table, light, light_array, load_meshs, load_model_materials, load_model_normals, compute_vertex_normals, load_scene, copy_rate, pack_tris_f16, record_order_verts, refit_nodes, scene_camera, standin_materials, view_from_camera)
from .host import (NO_TEXTURE, TEX_BILINEAR, TEX_NEAREST, TEX_RGBA8_SRGB, TEX_RGBA8_UNORM, TEXTURE_DESC_DTYPE, standin_texcoords,  # noqa: F401
                   standin_textures, texture_srgb_table, load_model_texcoords, load_model_material_maps)
