/*
 * trx.h — C-ABI of the MI355X (gfx950) CWBVH traversal backend for tray_racing.
 *
 * This is the drop-in boundary for the ONE hot path of DGriffin91/tray_racing:
 * closest-hit traversal of rays through a CWBVH (80-byte nodes) with
 * Moeller-Trumbore triangle tests, for primary and AO rays.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the tray_racing checkout; `query.hlsl` / `query_tlas.hlsl` are short for
 * src/rt_gpu/rt_gpu_software_query.hlsl / rt_gpu_software_query_tlas.hlsl, other
 * bare shader and .rs names live under src/rt_gpu/ or src/rt_cpu/).  Plain pointers and sizes only; no C++ or
 * torch types cross this boundary.  All functions return 0 on success or a
 * negative trx_status; the message is available from trx_last_error()
 * (thread-local).  Nothing here aborts: the Rust shim `expect()`s on the
 * status to keep the reference's panic convention (src/main.rs:178-180).
 *
 * There is NO CPU fallback behind this ABI: every trace entry point fails
 * with TRX_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef TRX_H
#define TRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRX_ABI_VERSION 1

typedef enum trx_status {
    TRX_OK = 0,
    TRX_ERR_INVALID = -1,        /* bad argument (null pointer, size mismatch, bad enum) */
    TRX_ERR_NO_DEVICE = -2,      /* no usable HIP device / HIP call failed               */
    TRX_ERR_OOM = -3,            /* host or device allocation failed                     */
    TRX_ERR_STACK_OVERFLOW = -4, /* a ray exceeded the traversal stack (result invalid)  */
    TRX_ERR_FORMAT = -5,         /* node/triangle buffer fails structural validation     */
    TRX_ERR_IO = -6              /* scene / model file could not be read                 */
} trx_status;

/* ---- data formats -------------------------------------------------------- */

/* One CWBVH node = 80 bytes = uint4[5], exactly the layout the reference's
 * GPU path consumes (src/rt_gpu/rt_gpu_software_query.hlsl:40-43, decode at
 * :219-224,249,257-264,381-384; size asserts src/rt_gpu/mod.rs:70,105;
 * writer embree/src/bvh_embree_to_cwbvh.rs:172-185). */
#define TRX_NODE_BYTES 80u

/* Triangle input formats accepted by trx_scene_create. */
typedef enum trx_tri_format {
    /* obvhs RtCompressedTriangle, 24 B: f32 v0[3]; u32 e[3] with
     * e[k] = f16(e2[k]) | f16(e1[k]) << 16, e1 = v1 - v0, e2 = v2 - v0
     * (src/rt_gpu/rt_gpu_software_query.hlsl:45-49,75-85; src/rt_gpu/mod.rs:39-43,86). */
    TRX_TRI_F16_24 = 0,
    /* Raw obvhs `Triangle`, 36 B: f32 v0[3], v1[3], v2[3] (src/main.rs:515-519,540-544). */
    TRX_TRI_VERTS_36 = 1,
    /* f32 {v0[3], e1[3], e2[3]}, 36 B with e1 = v0 - v1, e2 = v2 - v0: the
     * f32 content of obvhs RtTriangle without padding / ng (src/rt_cpu/mod.rs:38-43). */
    TRX_TRI_EDGES_36 = 2
} trx_tri_format;

/* Bytes per triangle for a trx_tri_format (0 for an unknown value). */
uint32_t trx_tri_format_bytes(uint32_t tri_format);

/* Traversal semantics (bit set).  0 is the literal in-tree HLSL text.  The
 * reference's --cpu path lives in the un-vendored obvhs crate; the deviations
 * recalled for it are exposed as bits, and TRX_SEM_CPU is
 * the preset that combines them.  Every combination has an oracle twin. */
typedef enum trx_semantics {
    /* per-node IEEE divides, separate multiply and add for the slab planes,
     * tt <= t commits (last equal-t triangle wins):
     * src/rt_gpu/rt_gpu_software_query.hlsl:237-242,285-286,120 */
    TRX_SEM_HLSL = 0,
    /* node test multiplies by inv_dir = 1/dir computed once per ray with an IEEE
     * divide.  2^e * inv_dir is bit-identical to 2^e / dir (power-of-two scale);
     * (p - origin) * inv_dir may differ from (p - origin) / dir in the last ulp,
     * which can only change which boxes are culled at razor edges. */
    TRX_SEM_NODE_RCP = 1u << 0,
    /* commit a triangle only if tt < t (first equal-t triangle wins) */
    TRX_SEM_TIE_FIRST = 1u << 1,
    /* evaluate the slab planes q * adj_inv + adj_origin with one fused
     * multiply-add (the HLSL leaves contraction to the compiler) */
    TRX_SEM_NODE_FMA = 1u << 2,
    /* recalled obvhs CPU path: precomputed inv_direction, strict t < tmax */
    TRX_SEM_CPU = (1u << 0) | (1u << 1)
} trx_semantics;

/* ViewUniform mirror (src/main.rs:589-597, HLSL cbuffer
 * src/rt_gpu/rt_gpu_software.hlsl:30-38).  Matrices are column-major like glam
 * (m[c*4 + r]).  Filled by trx_view_from_camera or by the caller. */
typedef struct trx_view {
    float view_inv[16];
    float proj_inv[16];
    float eye[3];
    float exposure;
    uint32_t tlas_start; /* unused by the traced path; scene carries it */
    uint32_t _pad[3];
} trx_view;

/* Explicit ray, 32 B: mirrors obvhs Ray::new(origin, direction, tmin, tmax)
 * as used at src/rt_cpu/rt_cpu.rs:50-55,76. */
typedef struct trx_ray {
    float origin[3];
    float tmin;
    float direction[3];
    float tmax;
} trx_ray;

/* Compact hit record written by every kernel: 8 B per ray.
 * Miss: t = +inf, prim = 0xFFFFFFFF (RayHit::none(), callers test
 * hit.t < f32::MAX, src/rt_cpu/rt_cpu.rs:61,82).  `prim` indexes the
 * triangle buffer handed to trx_scene_create (i.e. primitive_indices order,
 * src/rt_gpu/mod.rs:38-48). */
typedef struct trx_hit {
    float t;
    uint32_t prim;
} trx_hit;

/* Hit attributes, 24 B per hit record (trx_hit_attributes_*): what a renderer shades a hit with, beyond t and prim -
 * the reference's triangle test writes barycentric = float2(u, v) when it commits (query.hlsl:89-129), and its
 * Intersectable trait has compute_barycentric / compute_normal (traversable/src/lib.rs:31-43).
 *  u, v    the barycentrics the committing triangle test computed, over the 48-byte record {v0, e1 = v0 - v1,
 *          e2 = v2 - v0, ng = cross(e1, e2)}: c = v0 - o, r = cross(d, c), det = dot(ng, d), u = dot(r, e2) * (1 / det),
 *          v = dot(r, e1) * (1 / det), every dot (x*x' + y*y') + z*z' without contraction.  (o, d) is the ray that test
 *          saw: the world ray with every zero direction component replaced by FLT_EPSILON, or - on a scene with instance
 *          transforms - the world ray as given taken through the instance's world-to-object rows
 *          (trx_scene_get_instance_world_to_object) and then fixed the same way.
 *          Convention (DXR's): u weights v1 and v weights v2, the hit point is (1 - u - v) * v0 + u * v1 + v * v2.
 *  normal  the record's ng - with instance transforms first taken to world space by the transpose of the instance's
 *          world-to-object rows - times 1 / sqrtf(dot(ng, ng)): the world-space unit geometric normal, NOT flipped toward
 *          the ray (the AO pass's normal before its flip).
 * A record whose prim is not a triangle of the scene (a miss: prim = 0xFFFFFFFF), or whose instance id is outside the
 * instance table on a scene with instance transforms, gets all-zero bits.  t is not looked at. */
typedef struct trx_hit_attr {
    float u, v;
    float normal[3];
    uint32_t _pad; /* written as 0 */
} trx_hit_attr;

/* Mirror of obvhs RayHit {primitive_id, geometry_id, instance_id, t}
 * (fields: embree/src/embree_managed.rs:52-57) for the Traversable shim. */
typedef struct trx_rayhit {
    uint32_t primitive_id;
    uint32_t geometry_id;
    uint32_t instance_id;
    float t;
} trx_rayhit;

/* Which pixels of the w*h image this call (this GPU) traces: 8x8-pixel tiles
 * are numbered row-major; a call traces tiles with (tile % count) == index.
 * {0,1,0,0} = whole image.
 * layout 0 (TRX_LAYOUT_IMAGE): hit buffers are indexed by full-image pixel id
 * (y*w + x); pixels of other shards are left as they were.
 * layout 1 (TRX_LAYOUT_SHARD): hit buffers are compact, indexed by
 * local_tile*64 + (y&7)*8 + (x&7) with local_tile = tile / count; they hold
 * trx_shard_tiles() * 64 records (records of pixels outside the image are not
 * written).  This is the buffer a rank hands to the end-of-frame gather. */
#define TRX_LAYOUT_IMAGE 0u
#define TRX_LAYOUT_SHARD 1u
typedef struct trx_shard {
    uint32_t index;
    uint32_t count;
    uint32_t layout;
    uint32_t _pad;
} trx_shard;
/* Number of 8x8 tiles of a width x height image that belong to `shard`. */
uint32_t trx_shard_tiles(uint32_t width, uint32_t height, trx_shard shard);

/* Per-call counters (optional; pass NULL).  n_node / n_tri are the PROFILE_RT
 * counters of the reference (aabb_hit_count/8 and tri_hit_count,
 * src/rt_gpu/rt_gpu_software_query.hlsl:377-379,407-409), summed over rays. */
typedef struct trx_stats {
    uint64_t n_rays;
    uint64_t n_node;
    uint64_t n_tri;
    uint64_t n_hits;
    uint32_t max_stack;
    uint32_t overflow; /* number of rays that overflowed the stack */
    float kernel_ms;   /* hipEvent time of the traversal kernel(s) of this call */
    float _pad;
    /* wave-level executions of the node step / triangle test: n_node / (64 * n_wave_node)
     * is the SIMD efficiency of the node phase, likewise for triangles */
    uint64_t n_wave_node;
    uint64_t n_wave_tri;
} trx_stats;

typedef struct trx_scene trx_scene; /* opaque: device-resident nodes/tris/instances */

/* ---- errors / device ------------------------------------------------------ */

const char *trx_last_error(void);
uint32_t trx_abi_version(void);
/* Number of HIP devices visible (0 when none; never fails). */
int trx_device_count(void);
/* gcnArchName of a device into buf (e.g. "gfx950:sramecc+:xnack-"). */
int trx_device_name(int device, char *buf, size_t buf_len);

/* ---- scene upload ---------------------------------------------------------
 * Replaces the buffer upload half of rt_gpu_software::start
 * (src/rt_gpu/rt_gpu_software.rs:24-32 signature; :83-160 buffer creation),
 * fed by cwbvh_gpu_runner (src/rt_gpu/mod.rs:92-100 TLAS, :108-110 BLAS-only).
 *
 *  bvh_bytes        n_nodes * 80 bytes; all BLAS concatenated, TLAS last
 *  tri_bytes        n_tris * trx_tri_format_bytes(tri_format), in
 *                   primitive_indices order, primitive_base_idx pre-offset
 *  instance_offsets u32 BLAS node offset per TLAS primitive, or NULL / 0 when
 *                   there is no TLAS (the reference passes 16 zero bytes)
 *  tlas_start       node index of the TLAS root (0 and n_instances == 0 = BLAS only)
 *  device           HIP device ordinal
 * The inputs are copied; the caller keeps ownership. */
int trx_scene_create(const void *bvh_bytes, uint64_t n_nodes,
                     const void *tri_bytes, uint64_t n_tris, uint32_t tri_format,
                     const uint32_t *instance_offsets, uint32_t n_instances,
                     uint32_t tlas_start, int device, trx_scene **out);
void trx_scene_destroy(trx_scene *scene);
/* Bytes resident in HBM for this scene: nodes + 48-byte triangles + instances + what the launch slots used so far
 * hold (stack spill areas sized for the launched grids, tile-order lists). */
uint64_t trx_scene_device_bytes(const trx_scene *scene);
int trx_scene_device(const trx_scene *scene);

/* Optional: first triangle of each BLAS in the global triangle buffer
 * (n_blas + 1 entries, trx_flat.blas_tri_start) so trx_traverse1 can report
 * (geometry_id, local primitive_id) like the reference's CPU TLAS path
 * (src/cwbvh.rs:151-160). */
int trx_scene_set_geometry_ranges(trx_scene *scene, const uint32_t *blas_tri_start, uint32_t n_blas);

/* ---- entry nodes (TLAS scenes) -------------------------------------------------
 * In the reference a TLAS primitive is a whole BLAS: the walk enters at node 0 of the BLAS at instance_offsets[k]
 * (rt_gpu_software_query_tlas.hlsl:439-443).  entry_nodes[k] lets primitive k enter at another node of that BLAS
 * instead, so a TLAS can reference SUBTREES (re-braiding: a BLAS spanning the scene is opened into the pieces under its
 * root, trx_set_build_rebraid / trx_flat.instance_entry_nodes).  Several primitives may name the same BLAS; hit records
 * are unchanged (primitive ids are global, instance ids are TLAS primitives).  NULL / 0 restores node 0 everywhere; an
 * entry outside its BLAS is refused (TRX_ERR_FORMAT).  Buffers that come from the reference's host never need this. */
int trx_scene_set_instance_entry_nodes(trx_scene *scene, const uint32_t *entry_nodes, uint32_t n_instances);

/* ---- instance transforms (TLAS scenes) ----------------------------------------
 * The reference's TLAS path carries no transforms yet: "TODO transform ray according to the mesh transform"
 * (src/rt_gpu/rt_gpu_software_query_tlas.hlsl:409,433), "TODO Reset Ray to untransformed version" (:484), and
 * Traversable::get_instance_transform returns Mat4::default() (traversable/src/lib.rs:25-27, src/cwbvh.rs:163-165).
 * Here an instance is a TLAS primitive (entry k of instance_offsets): it may place its BLAS anywhere, and several
 * instances may share one BLAS.  object_to_world: n_instances column-major 4x4 affine matrices (glam Mat4 layout,
 * last row 0 0 0 1) in instance_offsets order; NULL / 0 restores identity.  On BLAS entry the ray is taken into
 * object space by the inverse (computed in double, rounded once to f32; origin as a point, direction as a vector,
 * NOT renormalised, so hit.t stays in world units); on exit the world ray is restored.  The TLAS node boxes handed
 * to trx_scene_create must bound the TRANSFORMED instances (trx_flat_build_instanced does that).  With no
 * transforms set the kernels behave exactly as before. */
int trx_scene_set_instance_transforms(trx_scene *scene, const float *object_to_world, uint32_t n_instances);
/* Traversable::get_instance_transform: the matrix given above, or identity. */
int trx_scene_get_instance_transform(const trx_scene *scene, uint32_t instance_id, float out_object_to_world[16]);
/* The world-to-object rows the kernels use: 3 rows of {m0 m1 m2 t}; x' = ((m0*x + m1*y) + m2*z) + t. */
int trx_scene_get_instance_world_to_object(const trx_scene *scene, uint32_t instance_id, float out_rows[12]);

/* ---- instance masks (TLAS scenes) ------------------------------------------------------------------------------------
 * The 8-bit instance mask of DXR / Vulkan instances (the reference's AccelerationStructureInstance packs one beside the
 * custom index; its software TLAS walk ignores it).  An instance is a TLAS primitive: entry k of instance_offsets, the
 * index the transforms and the hit records' instance ids use - per TLAS primitive on re-braided scenes too.
 *  - Every instance has a mask; with no table set every mask is 0xFF.
 *  - A MASKED call takes a ray_mask in 1..255 (0 or > 255: TRX_ERR_INVALID before anything is enqueued).  Instance k
 *    is considered only if (mask[k] & ray_mask) != 0.  An instance not considered is never entered: none of its
 *    triangles can be hit, and it has no effect on t, prim, the instance id, the occlusion flag or the AO pass.  A
 *    masked trace returns exactly what an unmasked trace returns on the same scene with those instances removed
 *    (tie-breaking under every semantics word included: the order of the TLAS walk does not change).
 *  - Only the masked entry points below read the table.  Every other entry point traces every instance whatever table
 *    is set: the primary, AO, frame, batch, rays, occluded and count calls, trx_frame_loop, trx_traverse1 /
 *    trx_traverse_batch (and the ray service behind them).
 *  - On single-level scenes the masked calls trace exactly what their unmasked twins trace (the scene is one instance
 *    with mask 0xFF), and the setter is refused (TRX_ERR_INVALID).
 *  - trx_scene_refit*, trx_scene_set_instance_transforms and trx_scene_set_instance_entry_nodes keep the table;
 *    trx_scene_device_bytes counts it.
 * n_instances must equal the scene's TLAS primitive count (TRX_ERR_INVALID otherwise).
 * Ordering: a masked launch enqueued before trx_scene_set_instance_masks uses the old table in full, one enqueued after
 * it returns the new one (the old table is freed once the scene's launches enqueued before the call have finished). */
/* masks: n_instances bytes; NULL / 0 removes the table (every instance 0xFF again). */
int trx_scene_set_instance_masks(trx_scene *scene, const uint8_t *masks, uint32_t n_instances);
/* The table as set, or 0xFF for every instance when none is (single-level scenes: n_instances 1, mask 0xFF). */
int trx_scene_get_instance_masks(const trx_scene *scene, uint8_t *out, uint32_t n_instances);
/* Masked forms of trx_trace_rays_inst_dev, trx_trace_occluded_dev, trx_trace_primary_inst_dev and
 * trx_trace_ao_inst_dev: the same arguments and rules (d_inst / d_ao_inst may be NULL; the AO call needs d_primary_inst
 * on scenes with instance transforms) plus ray_mask.  The AO pass takes the records of a primary pass - usually the
 * masked one - as they are: pixels whose primary record is a miss get a miss record.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_rays_masked_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, uint32_t semantics,
                              uint32_t ray_mask, trx_hit *d_hits, uint32_t *d_inst, void *stream);
int trx_trace_occluded_masked_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, uint32_t semantics,
                                  uint32_t ray_mask, uint8_t *d_flags, void *stream);
int trx_trace_primary_masked_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                 trx_shard shard, uint32_t semantics, uint32_t ray_mask, trx_hit *d_hits,
                                 uint32_t *d_inst, void *stream);
int trx_trace_ao_masked_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                            uint32_t semantics, uint32_t frame, float ao_eps, uint32_t ray_mask,
                            const trx_hit *d_primary, const uint32_t *d_primary_inst, trx_hit *d_ao, uint32_t *d_ao_inst,
                            void *stream);
/* Host-buffer forms (synchronous, like trx_trace_rays_inst / trx_trace_occluded; out_* may be NULL). */
int trx_trace_rays_masked(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics, uint32_t ray_mask,
                          trx_hit *out_hits, uint32_t *out_inst, float *out_ms);
int trx_trace_occluded_masked(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics,
                              uint32_t ray_mask, uint8_t *out_flags, float *out_ms);

/* ---- refit: geometry moves, topology stays ------------------------------------------------------------------------
 * A refit gives the scene new f32 vertices for every triangle record, in the scene's record order (the layout of
 * trx_flat.tri_verts, TRX_TRI_VERTS_36: 9 floats per record; object-order vertices map through trx_flat.tri_source),
 * and then
 *  - rewrites the 48-byte device triangle records exactly as trx_scene_create does for TRX_TRI_VERTS_36;
 *  - recomputes every node's quantisation frame (p, e) and the quantised bytes of every used child slot, bottom-up,
 *    with the builder's rules: a leaf child's box is the f32 min / max over the three vertices of each of its
 *    triangles; an inner child's box is the exact union of that child node's own child boxes (kept in f32, never
 *    decoded from the bytes); the frame and bytes follow the builder's encoder; a TLAS leaf child's box is the union of
 *    its primitives' boxes, primitive k's box being the refit box of BLAS node instance_offsets[k] + entry[k] - with
 *    instance transforms, its 8 corners taken through object_to_world[k] and padded as trx_flat_build_instanced pads
 *    them, without transforms used as it is (as trx_flat_build's TLAS does).
 * It keeps imask, child_base_idx, primitive_base_idx, child_meta, the bytes of empty slots, the instance table and the
 * entry nodes.  So a refit with the vertices (and transforms) a scene was built from returns its nodes byte for byte for
 * single-level builds without pre-splitting (trx_set_build_split(0), the default), trx_flat_build TLAS builds without
 * re-braiding (trx_set_build_rebraid(0)) and trx_flat_build_instanced scenes.  That holds for signed zeros too: a box
 * minimum over +0 and -0 keeps whichever the fold met first, and the builder folds in merge order where the refit folds in
 * slot order, so builder and refit both write a frame origin that is zero as +0 (never -0), whichever zero the box kept.
 * Pre-split and re-braided scenes get boxes
 * that bound everything they must but are not the build's bytes (a split reference gets its whole triangle's box, an
 * entry subtree its exact box instead of the decoded, outward-rounded one).  The tree was built for the old geometry:
 * walks cost more as the geometry moves away from it, and when to rebuild is the caller's decision.
 *
 * Moving instances: trx_scene_set_instance_transforms, then a refit (with the unchanged vertices) - the TLAS boxes then
 * bound the moved instances.  A vertex refit of a two-level scene refits its TLAS too.
 * Vertex normals (trx_scene_set_vertex_normals, below) are kept as they are: they are not recomputed from the new vertices, so a
 * caller whose refit changed the shape of the mesh sets the normals again.
 * Refused with TRX_ERR_INVALID, the scene left unchanged: a count other than the scene's triangle count, a null pointer,
 * a non-finite coordinate, a scene created from TRX_TRI_F16_24.
 * Ordering: every launch enqueued on the scene before the call sees the old geometry in full, every launch enqueued
 * after it returns the new one; both forms return once the refit has finished on the device.  The scene's ray services
 * (trx_traverse1) are stopped for the refit; callers arriving meanwhile wait and restart them. */
/* tri_verts (host memory): n_tris * 9 floats. */
int trx_scene_refit(trx_scene *scene, const float *tri_verts, uint64_t n_tris);
/* The same from device memory on the scene's device (e.g. a torch tensor), ordered on `stream` (NULL = null stream).
 * A pointer that is not a device allocation of the scene's device, or whose allocation ends before n_tris * 36 bytes,
 * is refused (TRX_ERR_INVALID) before anything reads it. */
int trx_scene_refit_dev(trx_scene *scene, const float *d_tri_verts, uint64_t n_tris, void *stream);
/* The node buffer as the kernels now see it (n_nodes * 80 B), for checking and for handing to other consumers. */
int trx_scene_read_nodes(trx_scene *scene, void *out_nodes, uint64_t n_nodes);
/* Host twin, no device needed: `nodes` (n_nodes * 80 B) refitted over tri_verts into out_nodes (may equal nodes), the
 * bytes trx_scene_refit produces.  instance_offsets / n_instances / tlas_start as for trx_scene_create; entry_nodes
 * (n_instances, or NULL = node 0) and object_to_world (n_instances column-major 4x4, or NULL = no transforms) as the
 * scene setters take them. */
int trx_refit_nodes(const void *nodes, uint64_t n_nodes, const float *tri_verts, uint64_t n_tris,
                    const uint32_t *instance_offsets, uint32_t n_instances, uint32_t tlas_start,
                    const uint32_t *entry_nodes, const float *object_to_world, void *out_nodes);

/* ---- what the trace calls accept ----------------------------------------------
 * Any bit pattern in a trx_ray or a trx_view: NaN, infinities, denormals, zero or un-normalised directions, tmin > tmax,
 * negative or NaN ranges.  The results are the reference shader's arithmetic on those floats (the oracle's, bit for bit:
 * tests/test_gpu_hostile_inputs.py), never a fault: no address depends on a ray's or a view's floats.  A non-finite or
 * out-of-range ray never changes another ray's record (it may send its wave through slower arithmetic: the literal
 * divisions), and it does not raise TRX_ERR_STACK_OVERFLOW: that error still means a tree deeper than 64 entries - or a
 * single ray that ran past the step cap of 2^22 trips, which only a whole-tree walker (below) over several million nodes
 * and triangles can reach.  The primary records and instance ids a caller hands to the passes after the trace: CALLER
 * RECORDS, below.
 *   What the shader's arithmetic does with such rays, because its node test is max(near planes, 0.0001) <= min(far planes,
 * t) with a max / min that drop NaN operands (query.hlsl:237-300):
 *   - a negative tmin is accepted by the triangle test but no hit nearer than a box's clamped entry is ever looked for:
 *     hits at t < 0.0001 are lost (a brute-force query would report them);
 *   - an origin on, or within a rounding of, a triangle's plane loses that nearest hit the same way;
 *   - a direction of length 2^12 or more shrinks every t by as much: hits nearer than 0.0001 in THOSE units are lost, and
 *     at 2^40 nothing is ever hit.  Directions are not renormalised inside an instance, so an instance whose transform
 *     scales the object-space direction past about 2^10 (a scale of 2^-10 or less, a near-singular shear) loses the near
 *     hits of its geometry, as the reference does;
 *   - a direction of length about 1e-38 has its hits at t near 1e38, where the box planes overflow first: they are lost;
 *   - a ray with a NaN on all three axes (any NaN in a view does that to every primary ray, through the normalisation)
 *     passes every box test and fails every triangle test: it reports a miss after visiting every node and testing every
 *     triangle of the scene.  Callers that cannot rule NaNs out should filter them: such a frame costs
 *     (nodes + triangles) per pixel.
 *
 * ---- CALLER RECORDS: the primary records and instance ids the later passes are handed ------------------------------
 * Several *_dev passes take a frame of primary records (d_primary), and the instance ids beside them (d_primary_inst),
 * from the caller and use the ids in them as indices into the scene's own tables.  Any bit pattern is accepted there as
 * well - a buffer nobody initialised, the records of another scene, an image-layout buffer of which one shard was traced
 * - and is never a fault: no address depends on a record's words.  The rule, stated once:
 *   - A primary record is a SURFACE RECORD of a scene iff t < FLT_MAX and prim < n_tris, n_tris being the extent given to
 *     trx_scene_create (0xFFFFFFFF is never below it: one unsigned comparison).  EVERY OTHER RECORD IS A MISS - NaN, +inf
 *     and FLT_MAX in t, any prim at or past the table's end - and the pass writes for that pixel exactly what it writes
 *     for a primary miss:
 *       the AO passes (trx_trace_ao_dev, _ao_inst_dev, _ao_batch_dev, _ao_masked_dev): the miss record {+inf, 0xFFFFFFFF},
 *         the instance id 0xFFFFFFFF;  trx_count_ao / trx_count_ao_per_ray: no ray - nothing counted, a zero trx_ray_cost;
 *       the ray writers (trx_ao_rays_dev, trx_light_rays_dev): the inert ray;
 *       the visibility passes (trx_trace_ao_visibility_dev, _sparse_dev, trx_trace_light_visibility_dev): TRX_AO_NO_SURFACE,
 *         the light pass in every light's plane;
 *       the indirect passes (trx_trace_indirect_dev, _sparse_dev): the base's bits (+0 without a base, and in the sparse form).
 *     A surface record is used as it stands, whatever walk or scene it came from: t may be negative or 0, prim need not be
 *     the triangle that pixel's primary ray hits.
 *   - On a scene with instance transforms an instance id >= n_instances selects no row: the hit triangle's object-space
 *     normal is used as it is - what 0xFFFFFFFF always meant.  Scenes without instance transforms never read the ids.
 *   - The attribute pass has its own rule for ids outside the tables: the zero record (trx_hit_attributes_*, below).
 *   - The passes that read no scene table - trx_ao_filter_dev, trx_ao_upsample_dev, trx_value_filter_dev,
 *     trx_value_upsample_dev, trx_light_term_dev and the shade calls - decide "surface" by t < FLT_MAX and
 *     prim != 0xFFFFFFFF: to them a record with a prim past the table is a surface pixel whose neighbours' terms it
 *     receives.  A caller who mixes the two families over foreign records gets each family's rule, not a fault.
 *   - No result changes for a record a trace call over the same scene wrote.
 * tests/test_gpu_caller_records.py holds every pass above to this over ids at, just past and far past the tables' ends
 * (tests/test_caller_records.py: the oracle and the twins).
 *
 * ---- SCENE SCALE: what a scene's size does to the passes after the trace ------------------------------------------
 * Multiply a scene by 2^k about the camera's eye (the eye at the origin) and every length the caller passes by 2^k too -
 * light positions and rect edges, shadow_eps, ao_eps, ao_radius, bounce_eps, a caller record's t.  That is the same
 * computation with every exponent shifted, so as long as nothing under- or overflows every output is an EXACT IMAGE of
 * the unit-scale one: barycentrics, normals, ray directions, cast decisions, wgeo, kinv, c, the selected emitters and the
 * 8-bit counts and filtered terms are the same bits; ray origins, tmax (not FLT_MAX, not the inert ray's -1), t and an
 * emitter record's V0, E1, E2 are multiplied by 2^k, its NG by 2^2k; the light term of point and rect lights by 2^-2k (a
 * directional light's and the ambient part are unchanged).  tests/test_scale.py computes the table ("scene
 * scale") on the twins; tests/test_gpu_scale.py holds the device to its own unit-scale output under it, and to the twins.
 * On the Cornell stand-in (triangle edges 0.0032 .. 1.34) every output above is exact for k = -20 .. +30: edges of about
 * 3e-9 .. 1.4e9.
 *   THE NORMAL LEAVES FIRST.  u and v of a carried record stay exact far beyond that range (k = -50 .. +62 on both test scenes); the unit normal does
 * not, because its intermediate dot(ng, ng), ng = cross(e1, e2), scales with the FOURTH power of the edge length: it is
 * a denormal below about 1.2e-38 (|ng|, twice the triangle's area, below 1.1e-19: edges of a few 1e-10) and +inf above
 * 3.4e38 (|ng| above 1.8e19: edges of a few 1e9).  On the stand-in the first normals lose bits at k = -26 (its smallest
 * edges at 4.8e-11), every dot(ng, ng) is a denormal at k = -32, the first normals are non-finite at k = -35 and all of
 * them from k = -38 on (1 / sqrtf(0) = +inf times ng: infinite and NaN components); upward the first normals are all-zero
 * at k = +33 (1 / sqrtf(+inf) = 0) and all of them at k = +48, until ng itself overflows (k = +68: NaN again).  The
 * arithmetic is the reference shader's and is not widened.  What the consumers then write, pinned by the same tests:
 *   - an all-zero normal faces nothing: trx_light_rays_dev, trx_bounce_light_rays_dev and trx_emitter_rays_dev write the
 *     inert ray, the light term keeps its ambient part alone, wgeo is +0, and no neighbour passes the filters' and
 *     upsamples' normal test (0 >= normal_cos fails): a pixel's filtered term is its own.  trx_ao_rays_dev still casts, along
 *     a finite direction;
 *   - a normal with NaN components fails every comparison likewise - the inert ray, +0, no accepted neighbour - and the AO
 *     ray's direction is NaN (such a ray hits nothing: "what the trace calls accept");
 *   - a normal that is infinite without a NaN component can pass a facing test: an ordinary shadow ray is cast and a
 *     directional light's term is +inf.  A caller who scales a scene that far has to expect +inf in the value plane.
 *   A PRIMARY WALK FINDS NOTHING once the whole scene is nearer than the node test's 0.0001 clamp (above): the stand-in at
 * k = -20 is all misses, while caller records carried to that scale are still served exactly.
 *
 * ---- camera ---------------------------------------------------------------
 * ViewUniform::from_camera (src/main.rs:602-616): proj_inv =
 * inverse(perspective_infinite_reverse_rh(fov_deg->rad, w/h, 0.01)),
 * view_inv = inverse(look_at_rh(eye, look_at, +Y)).
 * eye == look_at and a view direction parallel to +Y are refused with TRX_ERR_INVALID (*out holds no usable view: zeros
 * and a proj_inv); the reference's
 * unchecked from_camera returns a view_inv of NaNs there (the oracle's orc_view_from_camera does; tests/test_hostile_inputs.py),
 * and such a view, handed to a trace call as it is, hits nothing. */
int trx_view_from_camera(const float eye[3], const float look_at[3], float fov_deg,
                         float width, float height, trx_view *out);

/* ---- tracing: device-resident outputs --------------------------------------
 * `stream` is a hipStream_t (NULL = the null stream).  d_* pointers are device
 * memory on the scene's device.  These calls only enqueue work.
 *
 * Scheduling state (never results) lives with the stream: a stream keeps a launch slot of
 * the scene, and an image pass remembers, per image geometry, in which order its 8x8 tiles
 * are best started (heaviest first, learnt from the previous pass of that geometry on that
 * stream).  A frame loop that keeps its passes on one stream - as the reference does on its
 * one queue - gets that for free from the second frame on, camera motion and cuts included;
 * the first pass of a geometry, and a caller that sprays frames over many streams, run in
 * natural order (bench.py: 0.52 ms against 0.42 ms).  Hits are identical either way.
 *
 * trx_trace_primary_dev replaces the timed dispatch of the reference
 * (src/rt_gpu/rt_gpu_software.rs:289-302) restricted to the primary ray of
 * src/rt_gpu/rt_gpu_software.hlsl:69-89: ray-gen in-kernel, closest hit,
 * one trx_hit per pixel at d_hits[y*w + x]. */
int trx_trace_primary_dev(trx_scene *scene, const trx_view *view, uint32_t width,
                          uint32_t height, trx_shard shard, uint32_t semantics,
                          trx_hit *d_hits, void *stream);

/* The same with the instance (TLAS primitive index, RayHit.instance_id; 0xFFFFFFFF for a miss or a scene without
 * TLAS) each hit was found in: d_inst has one u32 per record, indexed like d_hits; may be NULL. */
int trx_trace_primary_inst_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                               trx_shard shard, uint32_t semantics, trx_hit *d_hits, uint32_t *d_inst, void *stream);

/* n_frames (1..TRX_MAX_BATCH_FRAMES) primary frames in ONE launch: frame f is traced with views[f] and its
 * records go to d_hits + f * frame_stride (in trx_hit records; frame_stride >= one frame's records for the
 * shard layout).  The reference renders frame after frame with one dispatch each
 * (src/rt_gpu/rt_gpu_software.rs:289-302); submitting several of them together gives the kernel's work queues
 * n_frames x the tiles to balance, which matters when a rank's share of one frame is small (tile shards on 8
 * GPUs: 4050 tiles for 4096 resident waves).  Results are identical to n_frames separate launches. */
#define TRX_MAX_BATCH_FRAMES 8
int trx_trace_primary_batch_dev(trx_scene *scene, const trx_view *views, uint32_t n_frames, uint32_t width,
                                uint32_t height, trx_shard shard, uint32_t semantics, trx_hit *d_hits,
                                uint64_t frame_stride, void *stream);

/* AO pass of src/rt_gpu/rt_gpu_software.hlsl:105-128 / src/rt_cpu/rt_cpu.rs:61-80:
 * for every pixel whose d_primary hit is valid, build the AO ray (normal from
 * the hit triangle flipped toward the viewer, origin = eye + d*t - d*ao_eps,
 * cosine-hemisphere direction from hash_noise(px, frame) /
 * hash_noise(px, frame + 1024)) and trace it (closest hit).  Pixels whose
 * primary ray missed get a miss record.  ao_eps: 0.0001 (GPU) / 0.01 (CPU).
 * The direction's sin / cos (sampling.hlsl:33-34 calls the platform's; on the CPU path Rust's f32::sin / cos are the C
 * library's sinf / cosf) are evaluated explicitly so that results reproduce bit for bit across machines: the binary64
 * algorithm the GNU C library (2.28 and later) publishes for sinf / cosf, rounded once to binary32 - measured identical to
 * glibc 2.35's sinf / cosf on x86_64 for every binary32 in [0, 2 pi] (tests/test_oracle.py; other glibc versions and
 * architectures pick other variants and may differ in the last bit), so on such a host the AO directions are the
 * reference CPU path's own.
 * Against a correctly rounded sin / cos (another C library) the AO hit's t moves in its last bits on a fraction of a
 * per cent of the rays.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_ao_dev(trx_scene *scene, const trx_view *view, uint32_t width,
                     uint32_t height, trx_shard shard, uint32_t semantics, uint32_t frame,
                     float ao_eps, const trx_hit *d_primary, trx_hit *d_ao, void *stream);

/* AO pass with instance ids: d_primary_inst (from trx_trace_primary_inst_dev) is REQUIRED when the scene has
 * instance transforms — the hit triangle's normal lives in object space and is taken to world space by the
 * transpose of the instance's world-to-object matrix; d_ao_inst may be NULL.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_ao_inst_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                          uint32_t semantics, uint32_t frame, float ao_eps, const trx_hit *d_primary,
                          const uint32_t *d_primary_inst, trx_hit *d_ao, uint32_t *d_ao_inst, void *stream);

/* The reference's whole pixel program as ONE launch (src/rt_gpu/rt_gpu_software.hlsl:47-144 is one dispatch: primary
 * ray, normal of the hit triangle, AO ray): d_primary / d_ao receive exactly what trx_trace_primary_inst_dev followed by
 * trx_trace_ao_inst_dev write (d_primary_inst / d_ao_inst may be NULL).  A lane whose primary ray ends in a hit becomes
 * that pixel's AO ray in place, so neither pass has a tail of its own and the primary hits never travel through memory. */
int trx_trace_frame_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                        uint32_t semantics, uint32_t frame, float ao_eps, trx_hit *d_primary, uint32_t *d_primary_inst,
                        trx_hit *d_ao, uint32_t *d_ao_inst, void *stream);

/* n_frames (1..TRX_MAX_BATCH_FRAMES) AO passes over ONE view and ONE primary hit buffer as one launch: pass f uses the
 * noise seed frame0 + f and writes its records at d_ao + f * frame_stride (d_ao_inst likewise, may be NULL;
 * d_primary_inst as for trx_trace_ao_inst_dev, NULL without instance transforms).  This is BASELINE.json's "4 spp":
 * the reference traces one AO ray per hit pixel per frame and varies the seed with the frame counter
 * (src/rt_cpu/rt_cpu.rs:95-97, src/rt_gpu/rt_gpu_software.rs:285-288), so 4 spp are frames 0..3 - submitted together
 * they share one launch's start-up and, above all, ONE drain (the end of an incoherent pass, where every wave finishes
 * its last rays at falling occupancy: two thirds of a hairball-class pass).  The seeds of a tile go to the same XCD.
 * Results are identical to n_frames separate trx_trace_ao_inst_dev launches.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_ao_batch_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                           uint32_t semantics, uint32_t frame0, uint32_t n_frames, float ao_eps,
                           const trx_hit *d_primary, const uint32_t *d_primary_inst, trx_hit *d_ao, uint32_t *d_ao_inst,
                           uint64_t frame_stride, void *stream);

/* Batch form of Traversable::traverse (traversable/src/lib.rs:13-28):
 * n explicit rays -> n hits. */
int trx_trace_rays_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays,
                       uint32_t semantics, trx_hit *d_hits, void *stream);

/* ... with the instance of every hit (d_inst: n u32, may be NULL). */
int trx_trace_rays_inst_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, uint32_t semantics,
                            trx_hit *d_hits, uint32_t *d_inst, void *stream);

/* Any-hit query — the reference's `intersects_bl_bvh` (query.hlsl:440-445; "Actual AO could use a faster
 * anyhit query", src/rt_cpu/rt_cpu.rs:78-79): one byte per ray, 1 if some triangle is hit inside
 * [tmin, tmax].  The traversal stops at the first accepted hit; until then it IS the closest-hit walk, so the
 * answer equals `trx_trace_rays*`'s hit / no hit exactly. */
int trx_trace_occluded_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays,
                           uint32_t semantics, uint8_t *d_flags, void *stream);

/* Hit attributes (trx_hit_attr) of hit records already traced: one 24-byte record per hit record, a post-pass that reads
 * the hits, rebuilds each ray and recomputes the committed triangle test's u, v and the normal.  The attributes depend
 * only on the committed triangle and the ray, so no semantics word is taken (under TRX_SEM_TIE_FIRST another triangle may
 * have been committed; its attributes follow it).
 *  d_inst  the instance id of every record (the *_inst_dev trace calls write them), REQUIRED when the scene has instance
 *          transforms - without it the call returns TRX_ERR_INVALID before anything is enqueued; ignored (may be NULL)
 *          on every other scene.
 * Ordering: these launches are ordered with trx_scene_refit* as trace launches are - a refit called after this call has
 * returned waits for the attribute pass, which sees the old geometry in full.
 * trx_hit_attributes_rays_dev: d_rays / d_hits / d_inst / d_attr hold n_rays records each (the hits of trx_trace_rays*_dev
 * over these rays, or any hit records over them). */
int trx_hit_attributes_rays_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, const trx_hit *d_hits,
                                const uint32_t *d_inst, trx_hit_attr *d_attr, void *stream);
/* The same for a primary frame: d_hits / d_inst laid out by `shard` exactly as trx_trace_primary*_dev wrote them (image
 * layout or TRX_LAYOUT_SHARD), d_attr laid out alike; the primary rays are regenerated from `view`.  In image layout the
 * records of pixels outside the shard are left untouched. */
int trx_hit_attributes_primary_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                   trx_shard shard, const trx_hit *d_hits, const uint32_t *d_inst, trx_hit_attr *d_attr,
                                   void *stream);

/* ---- AO visibility: any-hit AO rays with a radius, N samples per pixel -----------------------------------------------
 * The reference traces its AO ray with a closest-hit query "to create a bit more work for the benchmark" and notes that
 * "actual AO could use a faster anyhit query" (rt_gpu_software.hlsl:126-127, src/rt_cpu/rt_cpu.rs:78-79); the calls above
 * are that benchmark work.  These are what a renderer wants from the pass: per pixel, how many of n_samples AO rays of
 * bounded length reach nothing, without the records ever leaving the device.
 *
 * trx_ao_rays_dev writes the AO pass's rays as explicit rays: one trx_ray per record, records laid out exactly like the hit
 * buffers of trx_trace_ao_inst_dev for `shard` (image layout or TRX_LAYOUT_SHARD); records of pixels outside the shard or the
 * image are left untouched.  A pixel whose primary record is a hit gets, bit for bit, the ray trx_trace_ao_inst_dev builds
 * for it under seed `frame` (origin (eye + d*t) - d*ao_eps, cosine-hemisphere direction around the hit triangle's normal -
 * taken to world space through the instance's world-to-object rows when the scene has transforms - flipped toward the
 * viewer) with tmin = 0 and tmax = ao_radius.  ao_radius must be > 0; +inf is allowed and stored as FLT_MAX, which is what
 * the AO pass walks to; anything else (0, negative, NaN) is TRX_ERR_INVALID.  A pixel whose primary record is a miss
 * (!(t < FLT_MAX) or prim == 0xFFFFFFFF) gets the INERT ray: every word 0 except tmax = -1.0f - no walk can commit a hit on
 * it (closest-hit and any-hit kernels alike start from min(tmax, FLT_MAX)).  d_primary_inst is REQUIRED on scenes with
 * instance transforms, as for trx_trace_ao_inst_dev: without it the call returns TRX_ERR_INVALID before anything is enqueued.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_ao_rays_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                    uint32_t frame, float ao_eps, float ao_radius, const trx_hit *d_primary,
                    const uint32_t *d_primary_inst, trx_ray *d_rays, void *stream);
/* The visibility pass.  d_unoccluded holds one byte per record, laid out like the hit buffers: a pixel whose primary record
 * is a hit gets the number of samples f in 0..n_samples-1 whose AO ray - trx_ao_rays_dev's under seed frame0 + f - is NOT
 * occluded, "occluded" meaning that trx_trace_occluded_dev over that ray answers 1; a pixel whose primary record is a miss
 * gets TRX_AO_NO_SURFACE; records outside the shard or the image are untouched.  A renderer's AO term is count / n_samples.
 * n_samples outside 1..TRX_MAX_AO_SAMPLES, a bad radius and a missing d_primary_inst are refused (TRX_ERR_INVALID) before
 * anything is enqueued: the output is left as it was.
 * Everything runs on `stream` without host synchronisation: the rays of a chunk of tiles and samples are written into a
 * scratch the stream's launch slot of the scene owns ([tile][sample][64 pixels]: the samples of a tile lie together, at
 * most 288 MiB per slot, counted by trx_scene_device_bytes, released by trx_scene_destroy; growing it waits for the slot's
 * previous launch), the any-hit rays launch of trx_trace_occluded_dev walks them, a reduce kernel adds the flags into the
 * counts; chunk after chunk until every tile and sample is done.
 * Ordering: as for the other trace launches - a trx_scene_refit* called after this call has returned waits for the pass,
 * which sees the old geometry in full.  A stack overflow latches as for every rays launch (trx_scene_check).
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
#define TRX_MAX_AO_SAMPLES 64
#define TRX_AO_NO_SURFACE 0xFFu
int trx_trace_ao_visibility_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                trx_shard shard, uint32_t semantics, uint32_t frame0, uint32_t n_samples,
                                float ao_eps, float ao_radius, const trx_hit *d_primary,
                                const uint32_t *d_primary_inst, uint8_t *d_unoccluded, void *stream);

/* The SPARSE visibility pass: the visibility pass at one pixel in every stride x stride block.  Whole-image only: d_primary
 * and d_primary_inst are FULL-resolution image-layout records (y * width + x); there is no shard argument, for the reason
 * the filter below has none.  stride s is 1..TRX_MAX_AO_STRIDE, phase is 0..s*s-1 with px0 = phase % s, py0 = phase / s.
 * The low grid is Wlo = ceil(width / s) by Hlo = ceil(height / s) cells; d_unoccluded_lo holds Wlo * Hlo bytes in image
 * layout (Y * Wlo + X), nothing beyond them is written.  Cell (X, Y) stands for the full-resolution pixel
 * (X * s + px0, Y * s + py0): a cell whose pixel lies outside the image gets TRX_AO_NO_SURFACE, every other cell gets, byte
 * for byte, what trx_trace_ao_visibility_dev writes for that pixel under the same semantics, frame0, n_samples, ao_eps and
 * ao_radius - the rays are that pass's rays bit for bit (the ray direction and the noise are those of the full-resolution
 * pixel coordinates in the full width x height image; a low-resolution view does not give them).  A caller that rotates
 * phase over frames visits every pixel in s*s frames; stride 1 is the dense pass.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): stride 0 or above the maximum,
 * phase >= s*s, and everything trx_trace_ao_visibility_dev refuses - a missing d_primary_inst on a scene with instance
 * transforms among it.  Scratch, chunking, stream and ordering are the dense pass's: the same launch slot's scratch
 * ([tile][sample][64] over the 8 x 8 tiles of the low grid) under the same cap.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
#define TRX_MAX_AO_STRIDE 4
int trx_trace_ao_visibility_sparse_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                       uint32_t stride, uint32_t phase, uint32_t semantics, uint32_t frame0,
                                       uint32_t n_samples, float ao_eps, float ao_radius, const trx_hit *d_primary,
                                       const uint32_t *d_primary_inst, uint8_t *d_unoccluded_lo, void *stream);

/* ---- the frame's image: the AO term filtered, the frame shaded to RGBA8 on the device ------------------------------------
 * The reference's pixel program ends by storing a colour into an rgba8 output_texture in the same dispatch
 * (rt_gpu_software.hlsl:91,130-142).  These are the image passes after the walk: with them a frame leaves the device as
 * 4 bytes per pixel of finished image instead of 16 bytes per pixel of records.  None of them reads scene data; they take
 * the scene for its device and its launch order.
 * Ordering: as for the attribute pass - every launch takes a launch slot of the scene, so a trx_scene_refit* called after
 * one of these calls has returned waits for it.
 *
 * The edge-aware AO filter.  All buffers hold WHOLE-IMAGE records in image layout (y * width + x): what
 * trx_trace_primary*_dev, trx_hit_attributes_primary_dev and trx_trace_ao_visibility_dev write with shard {0, 1,
 * TRX_LAYOUT_IMAGE}.  There is no shard argument and no sharded form: a pixel's neighbours belong to other shards, and a
 * rank would need its neighbours' halo - a multi-GPU host filters after trx_assemble_frames.
 *  - A pixel p is a SURFACE pixel iff t_p < FLT_MAX and prim_p != 0xFFFFFFFF.  Any other pixel gets {0, 0}.
 *  - A surface pixel p gets the sums over the ACCEPTED pixels q of its (2 * radius + 1)^2 window clipped to the image:
 *    unoccluded = sum of d_unoccluded[q], samples = n_samples * (number of accepted q).  q is accepted iff it is a surface
 *    pixel, fabsf(t_q - t_p) <= depth_tol * t_p (every operation rounded once in binary32) and - with d_attr -
 *    (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_cos (no contraction); p itself is accepted unconditionally.
 *  - radius 0 gives {d_unoccluded[p], n_samples}.  The largest sum is 81 * 255: uint16_t cannot overflow.
 * Only the comparisons are done in float; the sums are integers.  A renderer's AO term is unoccluded / samples.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): radius > TRX_MAX_AO_FILTER_RADIUS,
 * n_samples outside 1..TRX_MAX_AO_SAMPLES, depth_tol negative or NaN (+inf allowed), normal_cos NaN, width * height == 0 or
 * beyond 2^31 - 1, a null scene, d_primary, d_unoccluded or d_term (d_attr may be NULL: no normal test). */
typedef struct trx_ao_term {
    uint16_t unoccluded;
    uint16_t samples;
} trx_ao_term;
#define TRX_MAX_AO_FILTER_RADIUS 4
int trx_ao_filter_dev(trx_scene *scene, uint32_t width, uint32_t height, const trx_hit *d_primary,
                      const trx_hit_attr *d_attr, const uint8_t *d_unoccluded, uint32_t n_samples, uint32_t radius,
                      float depth_tol, float normal_cos, trx_ao_term *d_term, void *stream);
/* The edge-aware UPSAMPLE of the sparse visibility pass: the full-resolution AO term rebuilt from the low grid's counts
 * under the filter's acceptance rule.  d_primary, d_attr (may be NULL: no normal test) and d_term are whole-image,
 * image-layout, FULL-resolution buffers; d_unoccluded_lo is what trx_trace_ao_visibility_sparse_dev wrote for the same
 * width, height, stride s and phase (Wlo * Hlo bytes, px0 = phase % s, py0 = phase / s).
 *  - Surface pixels are the filter's: t < FLT_MAX && prim != 0xFFFFFFFF.  Any other pixel gets {0, 0}.
 *  - The WINDOW of pixel p = (x, y) is the set of low cells (x / s + dx, y / s + dy) with |dx|, |dy| <= radius (integer
 *    divisions), clipped to the low grid.
 *  - Cell q is a SURFACE CELL iff its pixel (X * s + px0, Y * s + py0) is inside the image and is a surface pixel.
 *  - Cell q is ACCEPTED iff it is a surface cell, fabsf(t_q - t_p) <= depth_tol * t_p and - with d_attr -
 *    (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_cos: the filter's expressions, every operation rounded once
 *    in binary32, no contraction, t_q and n_q the full-resolution records of q's pixel.  The cell whose pixel is p itself
 *    is accepted unconditionally.
 *  - If at least one cell is accepted: unoccluded = the sum of the accepted cells' counts, samples = n_samples * (number
 *    of accepted cells).
 *  - FALLBACK: no cell is accepted but the window holds surface cells - the same sums over ALL surface cells of the window.
 *  - EMPTY: the window holds no surface cell - {0, 0}.
 * The largest sum is 25 * 255: uint16_t cannot overflow.  At stride 1 every pixel is its own cell and the terms are exactly
 * trx_ao_filter_dev's for the same radius.  Only the comparisons are done in float; the sums are integers.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): everything the filter refuses,
 * stride 0 or above TRX_MAX_AO_STRIDE, phase >= s*s, radius > TRX_MAX_AO_UPSAMPLE_RADIUS. */
#define TRX_MAX_AO_UPSAMPLE_RADIUS 2
int trx_ao_upsample_dev(trx_scene *scene, uint32_t width, uint32_t height, uint32_t stride, uint32_t phase,
                        const trx_hit *d_primary, const trx_hit_attr *d_attr, const uint8_t *d_unoccluded_lo,
                        uint32_t n_samples, uint32_t radius, float depth_tol, float normal_cos, trx_ao_term *d_term,
                        void *stream);
/* Shading to RGBA8: elementwise over n_records records in ANY layout (image or TRX_LAYOUT_SHARD; the output is laid out
 * like the input), 4 bytes {c, c, c, 255} per record at d_rgba (n_records * 4 bytes, 4-byte aligned; nothing beyond them is
 * written).  The colour per record, every division a single IEEE division:
 *   reference  the reference's shading (src/rt_cpu/rt_cpu.rs:57-85, the end of rt_gpu_software.hlsl): col = 1.0f / t where
 *              the primary record is a miss (!(t < FLT_MAX); 0 for t = +inf); on a hit col = ao.t / (1.0f + ao.t) where
 *              ao.t < FLT_MAX, 1 where the AO ray reached nothing.
 *   counts     TRX_AO_NO_SURFACE gives 0, otherwise col = (float)count / (float)n_samples (n_samples 1..TRX_MAX_AO_SAMPLES).
 *   term       samples == 0 gives 0, otherwise col = (float)unoccluded / (float)samples.
 * The code c is what the reference's host computes, on THIS host: (uint8_t)(uint32_t)(powf(col, 2.2f) * 255.0f), 0 for
 * col < 0 or NaN, 255 for col >= 1.  The device's powf is not the C library's, so the device evaluates no pow: at first
 * use the library derives thr[1..255], thr[k] the smallest binary32 in [0, 1] whose host code is >= k (bisection over the
 * bit pattern; thr[0] = 0), and on the device c is the number of k >= 1 with col >= thr[k].  trx_image_code_table hands the
 * table out (host only, no device needed).
 * Refused with TRX_ERR_INVALID before anything is enqueued: a null scene or - with n_records != 0 - a null buffer, a
 * misaligned d_rgba, n_samples outside its range.  n_records == 0 does nothing. */
int trx_image_code_table(float out_thresholds[256]);
int trx_shade_reference_dev(trx_scene *scene, const trx_hit *d_primary, const trx_hit *d_ao, uint64_t n_records,
                            uint8_t *d_rgba, void *stream);
int trx_shade_ao_counts_dev(trx_scene *scene, const uint8_t *d_unoccluded, uint32_t n_samples, uint64_t n_records,
                            uint8_t *d_rgba, void *stream);
int trx_shade_ao_term_dev(trx_scene *scene, const trx_ao_term *d_term, uint64_t n_records, uint8_t *d_rgba, void *stream);
/* Host-buffer form for a whole image (synchronous, serialised by the per-scene lock like its siblings): only the
 * width * height * 4 bytes of out_rgba (may be NULL) cross the bus; out_ms is the hipEvent time of all passes.
 *   n_samples == 0  the primary pass, the closest-hit AO pass under seed frame0, the reference shade (ao_radius,
 *                   filter_radius, depth_tol and normal_cos are not looked at): the image of trx_trace_primary_ao's records.
 *   n_samples >= 1  the primary pass and the AO visibility pass (seeds frame0 .., ao_radius as for
 *                   trx_trace_ao_visibility_dev); then with filter_radius == 0 the counts shade, with filter_radius >= 1
 *                   the attribute pass, the filter (with normals) and the term shade.
 * Every argument is validated before the first pass is enqueued. */
int trx_render_image(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                     uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius, uint32_t filter_radius,
                     float depth_tol, float normal_cos, uint8_t *out_rgba, float *out_ms);

/* trx_render_image with the AO term traced sparsely: the primary pass, the attribute pass, the sparse visibility pass at
 * (ao_stride, ao_phase), the upsample at upsample_radius with normals, the term shade; 4 bytes per pixel copied back.
 * n_samples is 1..TRX_MAX_AO_SAMPLES here.  Every argument is validated before the first pass is enqueued. */
int trx_render_image_sparse(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                            uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius, uint32_t ao_stride,
                            uint32_t ao_phase, uint32_t upsample_radius, float depth_tol, float normal_cos,
                            uint8_t *out_rgba, float *out_ms);

/* ---- direct light: masked shadow rays, the light term, the lit image ------------------------------------------------------
 * "Is this point lit": per pixel and light, shadow rays from the primary hit toward the light, walked by the any-hit rays
 * launch of trx_trace_occluded*_dev - with a ray mask, so that an instance can cast no shadow (trx_scene_set_instance_masks) -
 * then the usual split of direct lighting: the unshadowed analytic term times the traced visibility.  Intensities are
 * scalars: the image stays the reference's grey image.
 *
 * A light.  kind DIRECTIONAL: position = the direction TOWARD the light, any non-zero length.  POINT: position.  RECT:
 * position = a corner, the light is corner + u * edge1 + v * edge2, u, v in [0, 1].  _pad must be 0, every float finite. */
#define TRX_LIGHT_DIRECTIONAL 0u
#define TRX_LIGHT_POINT 1u
#define TRX_LIGHT_RECT 2u
#define TRX_MAX_LIGHTS 8
typedef struct trx_light {
    uint32_t kind;
    float position[3];
    float edge1[3];
    float edge2[3];
    float intensity;
    uint32_t _pad[5];
} trx_light;
/* THE SHADOW RAY of (pixel (px, py), light k, sample f).  Every operation is rounded once in binary32, no contraction;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *  - A pixel is a SURFACE pixel iff its primary record has t < FLT_MAX and prim != 0xFFFFFFFF (the AO pass's and the
 *    filter's rule).  Any other pixel gets the INERT ray of trx_ao_rays_dev: all words 0 except tmax = -1.0f.
 *  - d = the pixel's primary direction.  n = the hit triangle's geometric normal as trx_hit_attr.normal has it (the
 *    record's cross(e1, e2), through the instance's rows on a scene with instance transforms - d_primary_inst is REQUIRED
 *    there - times 1.0f / sqrtf(dot3(ng, ng))), flipped toward the viewer: n *= sg,
 *    sg = copysignf(1.0f, (n.x*-d.x + n.y*-d.y) + n.z*-d.z).
 *  - Origin: o[i] = (eye[i] + d[i]*t) - d[i]*shadow_eps.
 *  - Light point L: POINT: position.  RECT: u1 = hash_noise(px, py, seed), u2 = hash_noise(px, py, seed + 1024u) with
 *    seed = frame0 + k*64u + f and the AO ray's hash, L[i] = (position[i] + u1*edge1[i]) + u2*edge2[i].
 *  - POINT, RECT: v = L - o, q = dot3(v, v), dist = sqrtf(q), inv = 1.0f / dist, l = v * inv, tmax = fminf(dist, FLT_MAX).
 *    DIRECTIONAL: l = position * (1.0f / sqrtf(dot3(position, position))), tmax = FLT_MAX.  tmin = 0 either way.
 *  - Facing: c = dot3(n, l).  If !(c > 0.0f) the sample gets the inert ray and counts as NOT LIT: a light behind the
 *    surface, a light at the hit point (dist == 0 gives NaN), any NaN.
 *
 * trx_light_rays_dev writes the shadow rays of ONE light (`light`, whose index among the pass's lights is light_index) and
 * ONE sample as explicit rays: one trx_ray per record, laid out by `shard` exactly as for trx_ao_rays_dev; records outside
 * the shard or the image are left untouched.  Refused (TRX_ERR_INVALID, nothing enqueued): what the pass below refuses of
 * a light, light_index >= TRX_MAX_LIGHTS, sample >= TRX_MAX_AO_SAMPLES, a bad shadow_eps, null buffers, a missing
 * d_primary_inst on a scene with instance transforms.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_light_rays_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                       const trx_light *light, uint32_t light_index, uint32_t frame0, uint32_t sample, float shadow_eps,
                       const trx_hit *d_primary, const uint32_t *d_primary_inst, trx_ray *d_rays, void *stream);
/* The light visibility pass.  d_lit holds n_lights planes of `records` bytes, plane k at k * records, each laid out like
 * the hit buffers for `shard` (records = width * height in image layout, trx_shard_tiles() * 64 in TRX_LAYOUT_SHARD).  In
 * plane k a surface pixel gets the number of samples whose shadow ray toward light k was cast (not inert) and is NOT
 * occluded - "occluded" is what trx_trace_occluded_dev answers for that ray, with ray_mask != 0 what
 * trx_trace_occluded_masked_dev answers; a pixel without a surface gets TRX_AO_NO_SURFACE; records outside the shard or
 * the image are untouched.  POINT and DIRECTIONAL lights have one ray per pixel: it is traced once and their plane holds
 * 0 or 1 whatever n_samples is.  RECT lights take n_samples (1..TRX_MAX_AO_SAMPLES) samples f = 0..n_samples-1.
 * ray_mask 0: the unmasked launch, the instance mask table is not read; 1..255: the masked launch - an instance with
 * (mask & ray_mask) == 0 casts no shadow (on a single-level scene and on a scene without a table: the unmasked answer).
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): n_lights outside
 * 1..TRX_MAX_LIGHTS, an unknown kind, non-zero _pad, any non-finite light field, a directional light of zero length,
 * n_samples out of range, ray_mask > 255, shadow_eps NaN or negative, unknown semantics bits, null buffers, a missing
 * d_primary_inst on a scene with instance transforms.
 * Mechanics, stream and ordering are trx_trace_ao_visibility_dev's, once per light: the same launch slot's scratch
 * ([tile][sample][64]) under the same cap, the same chunk loops, no host synchronisation; a trx_scene_refit* called after
 * this call has returned waits for the pass.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_light_visibility_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                   trx_shard shard, uint32_t semantics, uint32_t ray_mask, const trx_light *lights,
                                   uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float shadow_eps,
                                   const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_lit, void *stream);
/* The light term: one float per record at d_value, laid out by `shard` like the other record buffers (d_primary, d_attr,
 * d_term and every plane of d_lit - planes at k * records as above - share that layout).  A pixel without a surface gets
 * 0.0f.  A surface pixel: n = d_attr.normal * sg (sg as above), P[i] = eye[i] + d[i]*t, E = ambient * a with a = 1.0f
 * when d_term is NULL, otherwise a = samples == 0 ? 0.0f : (float)unoccluded / (float)samples.  Then for k ascending:
 *   DIRECTIONAL  g = dot3(n, l), l as above.
 *   POINT, RECT  C = position (POINT) or C[i] = (position[i] + 0.5f*edge1[i]) + 0.5f*edge2[i] (RECT); v = C - P,
 *                q = dot3(v, v), inv = 1.0f / sqrtf(q), g = dot3(n, v*inv) / q.
 *   if g > 0.0f: E = E + (intensity_k * g) * ((float)count_k / (float)N_k), N_k = n_samples for a RECT light and 1
 *   otherwise, count_k = plane k's byte, TRX_AO_NO_SURFACE taken as 0.
 * Every operation rounded once in binary32, no contraction.  Refused (TRX_ERR_INVALID): what the visibility pass refuses of
 * lights, n_lights and n_samples, a non-finite ambient, null scene, view, d_primary, d_attr, d_lit or d_value. */
int trx_light_term_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                       const trx_light *lights, uint32_t n_lights, uint32_t n_samples, const trx_hit *d_primary,
                       const trx_hit_attr *d_attr, const uint8_t *d_lit, const trx_ao_term *d_term, float ambient,
                       float *d_value, void *stream);
/* Shading of float values to RGBA8: elementwise over n_records values in any layout, {c, c, c, 255} with c the code of the
 * value exactly as the other shades derive it (0 for negative or NaN, 255 for >= 1).  Refusals as for the other shades. */
int trx_shade_value_dev(trx_scene *scene, const float *d_value, uint64_t n_records, uint8_t *d_rgba, void *stream);
/* Host-buffer form for a whole image (synchronous, like trx_render_image): the primary pass, the attribute pass, the light
 * visibility pass (ray_mask, frame0, light_samples, shadow_eps), the light term and the value shade; with ao_samples >= 1
 * also the AO visibility pass (seeds frame0 .., ao_eps, ao_radius) and the filter at filter_radius (0..4, with normals),
 * whose term scales `ambient`; with ao_samples == 0 the ambient is unoccluded (ao_eps .. normal_cos are not looked at).
 * 4 bytes per pixel are copied back (out_rgba may be NULL), out_ms as for trx_render_image.  Every argument is validated
 * before the first pass is enqueued. */
int trx_render_image_lit(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                         uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                         uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                         float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos, uint8_t *out_rgba,
                         float *out_ms);

/* ---- indirect light: one diffuse bounce - bounce rays, lit secondary hits, the GI image --------------------------------------
 * The lit image shows only ambient * AO wherever no light reaches directly.  This pass adds what one diffuse bounce brings:
 * per pixel and sample a cosine-hemisphere ray from the primary hit, traced closest-hit, and at the surface it finds the
 * direct light of every light - a shadow ray and the analytic term, as above, with the bounce hit in the primary hit's place.
 * A composition of calls above: trx_ao_rays_dev's rays, trx_trace_rays_inst_dev's walk, trx_hit_attributes_rays_dev's
 * normals, trx_trace_occluded*_dev's any-hit walk.  Scalars throughout: the image stays grey.
 *
 * THE RULES, for the record of pixel (px, py), a sample f in 0..n_samples-1 (n_samples 1..TRX_MAX_AO_SAMPLES) and a light k.
 * Every operation is rounded once in binary32, no contraction; dot3 as above.
 *  1. BOUNCE RAY b_f: bit for bit the ray trx_ao_rays_dev writes for the pixel under seed frame0 + f with ao_eps = bounce_eps
 *     and ao_radius = +inf (its tmax is FLT_MAX).  A pixel that is not a surface pixel gets the inert ray (tmax < 0 marks it).
 *  2. BOUNCE HIT: what trx_trace_rays_inst_dev answers for b_f under `semantics` - closest-hit and UNMASKED: the mask applies
 *     to the shadow rays only, as above.  The bounce HAS A SURFACE iff b_f is not inert, t < FLT_MAX and prim != 0xFFFFFFFF.
 *     Its attribute record `attr` is what trx_hit_attributes_rays_dev writes for (ray, hit, instance id).
 *  3. SECONDARY SHADOW RAY: the shadow ray above with the primary hit replaced by the bounce hit.  d = b_f's direction,
 *     n = attr.normal * copysignf(1.0f, dot3(attr.normal, -d)), Q[i] = b_f.origin[i] + d[i]*t,
 *     o[i] = Q[i] - d[i]*shadow_eps; the light point L, l, tmax and the facing test are THE SHADOW RAY's statements.  A rect
 *     light takes ONE sample per bounce: u1 = hash_noise(px, py, seed), u2 = hash_noise(px, py, seed + 1024u) with
 *     seed = frame0 + k*64u + f.  Where the bounce has no surface, or !(dot3(n, l) > 0.0f), the ray is the inert ray and
 *     contributes nothing.
 *  4. WEIGHT: g_k is trx_light_term_dev's g with P := Q and the flipped n above (DIRECTIONAL: g = dot3(n, l); POINT, RECT:
 *     toward the centre C: v = C - Q, q = dot3(v, v), inv = 1.0f / sqrtf(q), g = dot3(n, v*inv) / q).  s_f = 0.0f; for k
 *     ascending: if the shadow ray was cast and is NOT occluded and g_k > 0.0f then s_f = s_f + intensity_k * g_k.  "Not
 *     occluded" is what trx_trace_occluded_dev answers for the ray, with ray_mask 1..255 what trx_trace_occluded_masked_dev
 *     answers.
 *  5. TERM: A = 0.0f; for f ascending: A = A + s_f.  out = base + (bounce_albedo * A) / (float)n_samples with
 *     base = d_base[record], or 0.0f when d_base is NULL.  A pixel without a surface gets base.  The order holds whatever the
 *     chunking.
 *
 * trx_bounce_light_rays_dev writes the secondary shadow rays of ONE light and ONE sample as explicit rays, so that all 32
 * bytes of every ray can be held to rule 3: d_bounce_rays, d_bounce_hits, d_bounce_attr and d_rays hold one record per record
 * of `shard`, laid out like every record buffer; records outside the shard or the image are untouched.  It takes no view and
 * no instance ids: the attribute record carries the world-space normal.  Refused (TRX_ERR_INVALID, nothing enqueued): what
 * trx_light_rays_dev refuses of light, light_index, sample and shadow_eps, an empty image or a bad shard, null buffers. */
int trx_bounce_light_rays_dev(trx_scene *scene, uint32_t width, uint32_t height, trx_shard shard, const trx_light *light,
                              uint32_t light_index, uint32_t frame0, uint32_t sample, float shadow_eps,
                              const trx_ray *d_bounce_rays, const trx_hit *d_bounce_hits,
                              const trx_hit_attr *d_bounce_attr, trx_ray *d_rays, void *stream);
/* The pass: one float per record at d_value (rule 5), laid out by `shard` like d_primary and d_primary_inst; records outside
 * the shard or the image are untouched.  d_base may be NULL, a buffer laid out alike, or d_value itself (every record's base
 * is read before its value is written; the running sums sit in the pass's scratch).
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): everything
 * trx_trace_light_visibility_dev refuses (lights, n_lights, ray_mask, shadow_eps, semantics bits, a missing d_primary_inst on
 * a scene with instance transforms), n_samples outside 1..TRX_MAX_AO_SAMPLES, bounce_eps NaN or negative, a non-finite
 * bounce_albedo, a null scene, view, d_primary or d_value.
 * Mechanics: everything runs on `stream` without host synchronisation.  Per chunk of tiles and samples ([tile][sample][64
 * pixels], as for trx_trace_ao_visibility_dev): the bounce rays, the closest-hit rays launch with instance ids, the attribute
 * pass in rays mode; then light after light the shadow rays, the any-hit rays launch (masked when ray_mask != 0) and the
 * weights; then the samples' sums are added to the tile's running sums.  Sample chunks and lights ascend, so rule 5's order
 * holds under any cap.  The scratch (about 6.8 KiB per tile and sample) belongs to the stream's launch slot of the scene,
 * shares the AO pass's rays and flags and its cap (288 MiB per slot), is counted once by trx_scene_device_bytes and
 * released by trx_scene_destroy; growing it waits for the slot's previous launch.
 * Ordering: as for the other passes - a trx_scene_refit* called after this call has returned waits for every launch of the
 * pass, which sees the old geometry in full.  A stack overflow latches as for every rays launch (trx_scene_check).
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_indirect_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                           uint32_t semantics, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                           uint32_t frame0, uint32_t n_samples, float bounce_eps, float shadow_eps, float bounce_albedo,
                           const trx_hit *d_primary, const uint32_t *d_primary_inst, const float *d_base, float *d_value,
                           void *stream);
/* trx_render_image_lit with one bounce: its passes up to the light term, then trx_trace_indirect_dev (bounce_samples
 * 1..TRX_MAX_AO_SAMPLES, seeds frame0 .., bounce_eps, bounce_albedo; the lights, ray_mask and shadow_eps of the direct pass)
 * with the light term's values as d_base and d_value, then the value shade.  4 bytes per pixel are copied back (out_rgba may
 * be NULL).  Every argument is validated before the first pass is enqueued. */
int trx_render_image_gi(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                        uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                        uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                        float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos,
                        uint32_t bounce_samples, float bounce_eps, float bounce_albedo, uint8_t *out_rgba, float *out_ms);

/* ---- the value filter: an edge-aware a-trous filter over a per-pixel float plane ----------------------------------------------
 * At an affordable sample count the indirect term is Monte-Carlo noise.  This is the filter for it - and for any other
 * per-pixel float plane: n_levels passes of a 5 x 5 B3-spline kernel whose taps lie 1, 2, 4, 8, 16 pixels apart, each tap
 * taken only where the primary record's depth and the attribute record's normal say it lies on the pixel's own surface (the AO
 * filter's acceptance rule).  All buffers hold WHOLE-IMAGE records in image layout (y * width + x); there is no shard argument
 * and no sharded form, for the reason trx_ao_filter_dev has none.  None of it reads scene data.
 *
 * THE RULES.  Every operation is rounded once in binary32, no contraction, every division a single IEEE division.
 *  - A pixel p is a SURFACE pixel iff t_p < FLT_MAX and prim_p != 0xFFFFFFFF (the AO filter's rule).
 *  - LEVEL j (0 .. n_levels-1) has spacing s = 1 << j and maps a plane u to a plane u':
 *      a pixel that is not a surface pixel gets u'[p] = u[p], its bits copied;
 *      a surface pixel p = (x, y) starts from num = 0.0f, den = 0.0f and visits its taps for dy = -2..2 ascending and, inside
 *      that, dx = -2..2 ascending: the tap is q = (x + dx*s, y + dy*s), its weight w = k[dy+2] * k[dx+2] with
 *      k = {1, 4, 6, 4, 1} - one of the integers 1, 4, 6, 16, 24, 36 as a float.  A tap outside the image is skipped.  A tap is
 *      ACCEPTED iff q is a surface pixel, fabsf(t_q - t_p) <= depth_tol * t_p and - with d_attr -
 *      (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_cos (the AO filter's expressions); p itself is accepted
 *      unconditionally.  For an accepted tap: num = num + w * u[q]; den = den + w (den is an exact integer, at most 256).
 *      u'[p] = num / den.
 *  - THE PASS: u_0 = d_in, the levels are applied in ascending order, F = u_{n_levels}.  A surface pixel gets base + F (one
 *    addition) with base = d_base[p], or F when d_base is NULL.  A pixel without a surface gets d_base[p], its bits copied, or
 *    d_in[p] when d_base is NULL.
 * Buffers: d_work holds width * height floats of the caller's; it is required when n_levels >= 2, may be NULL otherwise, and
 * its contents afterwards are unspecified.  Nothing beyond width * height floats of d_out or d_work is written.  d_base may be
 * d_out (every pixel's base is read before its value is written, and no earlier level writes d_out then: from three levels on
 * the second intermediate plane of such a call sits in a plane of width * height floats that the stream's launch slot of the
 * scene owns - counted by trx_scene_device_bytes, released by trx_scene_destroy; growing it waits for the slot's previous
 * launch).  d_in is never written.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): n_levels 0 or above
 * TRX_MAX_VALUE_FILTER_LEVELS, depth_tol negative or NaN (+inf allowed), normal_cos NaN, width * height == 0 or beyond
 * 2^31 - 1, a null scene, d_primary, d_in or d_out (d_attr may be NULL: no normal test), a null d_work with n_levels >= 2,
 * d_in == d_out, d_work equal to d_in, d_out or d_base.
 * Ordering: one launch per level on `stream`, no host synchronisation; every launch takes a launch slot of the scene, as the
 * other image passes do, so a trx_scene_refit* called after this call has returned waits for it. */
#define TRX_MAX_VALUE_FILTER_LEVELS 5
int trx_value_filter_dev(trx_scene *scene, uint32_t width, uint32_t height, const trx_hit *d_primary,
                         const trx_hit_attr *d_attr, const float *d_in, const float *d_base, uint32_t n_levels,
                         float depth_tol, float normal_cos, float *d_work, float *d_out, void *stream);
/* trx_render_image_gi with the indirect term filtered: the lit chain up to the light term V, trx_trace_indirect_dev without a
 * base into a plane I, trx_value_filter_dev over I (bounce_filter_levels 0..TRX_MAX_VALUE_FILTER_LEVELS, bounce_depth_tol,
 * bounce_normal_cos, the attribute pass's normals) with d_base = d_out = V, the value shade; 4 bytes per pixel are copied back
 * (out_rgba may be NULL).  bounce_filter_levels == 0 is trx_render_image_gi itself (the two tolerances are not looked at).
 * Every argument is validated before the first pass is enqueued. */
int trx_render_image_gi_filtered(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                                 uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                 uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                                 float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos,
                                 uint32_t bounce_samples, float bounce_eps, float bounce_albedo, uint32_t bounce_filter_levels,
                                 float bounce_depth_tol, float bounce_normal_cos, uint8_t *out_rgba, float *out_ms);

/* ---- the sparse indirect term: one bounce pixel in every stride x stride block, upsampled edge-aware ---------------------------
 * The indirect pass is the most expensive pass here, and most of it is the closest-hit walk over incoherent rays: the remedy
 * is fewer rays.  This is the sparse visibility pass's form for the indirect term: trx_trace_indirect_sparse_dev traces the
 * term over a low grid, trx_value_upsample_dev rebuilds a full-resolution plane from it under the filter's depth and normal
 * rule, and trx_value_filter_dev may follow.
 *
 * THE SPARSE PASS.  Whole-image and image-layout, without a shard argument, like trx_trace_ao_visibility_sparse_dev, and
 * with that call's grid: stride s is 1..TRX_MAX_AO_STRIDE, phase is 0..s*s-1 with px0 = phase % s, py0 = phase / s; the low
 * grid is Wlo = ceil(width / s) by Hlo = ceil(height / s) cells; d_value_lo holds Wlo * Hlo floats at Y * Wlo + X, nothing
 * beyond them is written; cell (X, Y) stands for the full-resolution pixel (X * s + px0, Y * s + py0).  d_primary and
 * d_primary_inst are FULL-resolution image-layout records.
 *  - A cell whose pixel lies outside the image, or whose pixel is not a surface pixel, gets +0.0f.
 *  - Every other cell gets, bit for bit, what trx_trace_indirect_dev writes for that pixel with d_base == NULL under the same
 *    arguments: the bounce ray is rule 1's for the full-resolution pixel coordinates in the full image, the rect light's
 *    noise of rule 3 is hash_noise(px, py, ...) of the full-resolution pixel, not of the cell, and the sums are formed in
 *    rule 4's and rule 5's order under any scratch cap.  Stride 1 is the dense pass without a base.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): stride 0 or above the maximum,
 * phase >= s*s, everything trx_trace_indirect_dev refuses, a null d_value_lo.  Scratch, chunking, stream and ordering are the
 * dense pass's: the same launch slot's scratch ([tile][sample][64] over the 8 x 8 tiles of the low grid) under the same cap,
 * counted once by trx_scene_device_bytes; a trx_scene_refit* called after this call has returned waits for every launch.
 * d_primary (and d_primary_inst) may hold any bit pattern: a record that is no surface record of this scene is a miss
 * (CALLER RECORDS, above). */
int trx_trace_indirect_sparse_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                  uint32_t stride, uint32_t phase, uint32_t semantics, uint32_t ray_mask,
                                  const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                  float bounce_eps, float shadow_eps, float bounce_albedo, const trx_hit *d_primary,
                                  const uint32_t *d_primary_inst, float *d_value_lo, void *stream);
/* THE UPSAMPLE of a low-grid float plane.  d_primary, d_attr (may be NULL: no normal test), d_base (may be NULL) and d_out
 * are full-resolution, whole-image, image-layout buffers; d_in_lo is a Wlo x Hlo plane of floats for the same width, height,
 * stride s and phase.  Every operation is rounded once in binary32, no contraction, every division a single IEEE division.
 *  - Surface pixels are the filter's: t < FLT_MAX && prim != 0xFFFFFFFF.
 *  - The WINDOW of pixel p = (x, y) is the set of low cells (x / s + dx, y / s + dy) with |dx|, |dy| <= radius (integer
 *    divisions; radius 0..TRX_MAX_VALUE_UPSAMPLE_RADIUS), clipped to the low grid: trx_ao_upsample_dev's window.
 *  - The cells are visited for dy ascending and, inside that, dx ascending.  The weight of a cell is w = k[|dy|] * k[|dx|]
 *    with k[d] = radius + 1 - d: an exact small integer as a float, at most 9.
 *  - Cell q is a SURFACE CELL iff its pixel (X * s + px0, Y * s + py0) is inside the image and is a surface pixel.
 *  - Cell q is ACCEPTED iff it is a surface cell, fabsf(t_q - t_p) <= depth_tol * t_p and - with d_attr -
 *    (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_cos, t_q and n_q the full-resolution records of q's pixel
 *    (trx_ao_upsample_dev's statements).  The cell whose pixel is p itself is accepted unconditionally.
 *  - num = 0.0f, den = 0.0f; for every accepted cell in the visit order: num = num + w * u[q]; den = den + w.  A cell that is
 *    not accepted leaves both as they are: a NaN or an infinity at a rejected cell stays out.
 *  - At least one cell accepted: F = num / den.  FALLBACK - none accepted but the window holds surface cells: the same two
 *    sums over ALL surface cells of the window, in the same order with the same weights, then F = num / den.  EMPTY - no
 *    surface cell in the window: F = +0.0f.
 *  - A surface pixel gets base + F (one addition) with base = d_base[p], or F when d_base is NULL.  A pixel without a surface
 *    gets d_base[p], its bits copied, or +0.0f without a base.  d_base may be d_out (every pixel's base is read before its
 *    value is written).
 * At stride 1 and radius 0 every surface pixel gets its own cell's value (u / 1.0f).
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): stride 0 or above TRX_MAX_AO_STRIDE,
 * phase >= s*s, radius > TRX_MAX_VALUE_UPSAMPLE_RADIUS, depth_tol negative or NaN (+inf allowed), normal_cos NaN,
 * width * height == 0 or beyond 2^31 - 1, a null scene, d_primary, d_in_lo or d_out, d_in_lo == d_out.
 * Ordering: one launch on `stream`, taking a launch slot of the scene like the other image passes. */
#define TRX_MAX_VALUE_UPSAMPLE_RADIUS 2
int trx_value_upsample_dev(trx_scene *scene, uint32_t width, uint32_t height, uint32_t stride, uint32_t phase,
                           const trx_hit *d_primary, const trx_hit_attr *d_attr, const float *d_in_lo, const float *d_base,
                           uint32_t radius, float depth_tol, float normal_cos, float *d_out, void *stream);
/* trx_render_image_gi_filtered with the indirect term traced sparsely: the lit chain up to the light term V,
 * trx_trace_indirect_sparse_dev (bounce_stride, bounce_phase) into a low plane; with bounce_filter_levels == 0
 * trx_value_upsample_dev (bounce_upsample_radius, bounce_depth_tol, bounce_normal_cos, the attribute pass's normals) with
 * d_base = d_out = V; otherwise the upsample without a base into a plane I and trx_value_filter_dev over I with
 * d_base = d_out = V; then the value shade; 4 bytes per pixel are copied back (out_rgba may be NULL).  The two tolerances are
 * looked at in either case: the upsample uses them.  Every argument is validated before the first pass is enqueued. */
int trx_render_image_gi_sparse(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                               uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                               uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                               float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos,
                               uint32_t bounce_samples, float bounce_eps, float bounce_albedo, uint32_t bounce_filter_levels,
                               float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase,
                               uint32_t bounce_upsample_radius, uint8_t *out_rgba, float *out_ms);

/* ---- materials and the colour image: per-triangle albedo and emission, the RGB bounce, compose, the RGB shade --------------------
 * Everything above is scalar.  What a bounce exists to carry is the colour of the surface it left: this section gives a scene
 * a material table keyed by trx_hit.prim, carries it through the indirect pass as three planes, and composes and shades a
 * colour image.  Purely additive: every call above computes what it computed.  Lights stay scalar (white).
 *
 * A material is a diffuse albedo and an emission, linear RGB.  tri_material[i] is the material of triangle i of the buffer
 * handed to trx_scene_create - `prim` order; a caller with a trx_flat applies tri_source.  On a two-level scene the instances
 * of a BLAS share its triangles' materials.
 * trx_scene_set_materials validates on the host before anything is copied and refuses with TRX_ERR_INVALID: a null pointer,
 * n_materials outside 1..TRX_MAX_MATERIALS, n_tris different from the scene's, any index >= n_materials, any albedo or
 * emission component that is negative or not finite.  Every index is checked here, so no kernel reads past the material
 * table.  Both tables are owned like the instance mask table: counted by trx_scene_device_bytes (24 B per material, 2 B per
 * triangle), kept by a refit, released by trx_scene_destroy; a second call replaces them after waiting for the scene's
 * launches in flight, which see the old tables in full; a refused call leaves the old tables in force.  A call whose
 * n_materials differs from the table it replaces also drops the scene's texture set (trx_scene_set_textures, below), which is
 * keyed by material.
 * trx_scene_get_materials: *inout_n_materials holds the capacity of out_materials on entry and the table's size on return;
 * refused on a scene without materials, with a capacity below the size, or with n_tris different from the scene's.
 * Every colour entry point below is refused with TRX_ERR_INVALID on a scene without materials. */
typedef struct trx_material {
    float albedo[3];
    float emission[3];
} trx_material; /* 24 B */
#define TRX_MAX_MATERIALS 65536u
int trx_scene_set_materials(trx_scene *scene, const trx_material *materials, uint32_t n_materials,
                            const uint16_t *tri_material, uint64_t n_tris);
int trx_scene_get_materials(const trx_scene *scene, trx_material *out_materials, uint32_t *inout_n_materials,
                            uint16_t *out_tri_material, uint64_t n_tris);

/* THE RGB INDIRECT TERM.  trx_trace_indirect_dev with the launch-wide bounce_albedo replaced by the material of the triangle
 * every bounce ray hits.  Rules 1 to 4 of "indirect light" hold unchanged: bounce ray, bounce hit, secondary shadow rays and
 * s_f are bit for bit those of trx_trace_indirect_dev.  In rule 5's place:
 *  5c. Every operation is rounded once in binary32, no contraction.  A_c = 0.0f for c = 0 (R), 1 (G), 2 (B).  For f
 *      ascending: if bounce f has a surface (rule 2), m = tri_material[bounce_hit_f.prim] and for each c
 *      A_c = A_c + (albedo_c(m) * s_f + emission_c(m)) - one multiplication and two additions, in that association; a bounce
 *      without a surface leaves A_c as it is.  out_c = A_c / (float)n_samples, a single IEEE division.  A record that is no
 *      surface record gets +0.0f in all three planes; a record outside the shard or the image is untouched.  The order holds
 *      under any scratch cap.  Emission is two-sided: there is no facing test.
 * d_value_rgb holds three planes of floats, plane c at c * records, each laid out by `shard` like d_primary; records follows
 * trx_trace_light_visibility_dev's plane rule (width * height in image layout, trx_shard_tiles() * 64 in TRX_LAYOUT_SHARD).
 * There is no base and no bounce_albedo.  The sparse form is trx_trace_indirect_sparse_dev's statement: its grid and phase,
 * plane c at c * Wlo * Hlo, every cell bit for bit the dense value of its full-resolution pixel, +0 in all three planes for a
 * cell whose pixel leaves the image or is no surface pixel; stride 1 is the dense pass in image layout.
 * Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it was): everything the grey pass refuses, a
 * scene without materials, a null output.  Mechanics, scratch, cap, stream and ordering are the grey pass's; the running sums
 * are three per tile pixel.  An emissive triangle is seen by bounce rays (and directly, below); it is no sampled light. */
int trx_trace_indirect_rgb_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                               uint32_t semantics, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                               uint32_t frame0, uint32_t n_samples, float bounce_eps, float shadow_eps,
                               const trx_hit *d_primary, const uint32_t *d_primary_inst, float *d_value_rgb, void *stream);
int trx_trace_indirect_rgb_sparse_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                      uint32_t stride, uint32_t phase, uint32_t semantics, uint32_t ray_mask,
                                      const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                      float bounce_eps, float shadow_eps, const trx_hit *d_primary,
                                      const uint32_t *d_primary_inst, float *d_value_rgb_lo, void *stream);

/* COMPOSE AND SHADE.  Both are elementwise over n_records records in any layout; planes lie at c * n_records.
 * trx_material_compose_dev: a record with t < FLT_MAX, prim != 0xFFFFFFFF and prim < n_tris has m = tri_material[prim] and
 * colour_c = emission_c(m) + albedo_c(m) * (E + I_c) with E = d_direct[r] (trx_light_term_dev's scalar plane, AO-scaled ambient
 * included) and I_c = d_indirect_rgb[c * n_records + r]: the inner addition, then the multiplication, then the addition, each
 * rounded once in binary32.  With d_indirect_rgb == NULL it is emission_c(m) + albedo_c(m) * E.  Any other record is
 * background: +0.0f in all three planes (CALLER RECORDS, above).  d_colour_rgb may be d_indirect_rgb: each lane reads before
 * it writes.  The primary albedo multiplies here, after any filter: trx_value_upsample_dev and trx_value_filter_dev run on the
 * demodulated I_c, one call per plane - why the layout is planar.  Refused (TRX_ERR_INVALID): a null scene, d_primary,
 * d_direct or d_colour_rgb, n_records == 0 or beyond 2^31 - 1, a scene without materials.
 * trx_shade_rgb_dev: {code(R), code(G), code(B), 255} per record, code derived exactly as trx_shade_value_dev derives it - the
 * same threshold table, 0 for negative or NaN, 255 for >= 1.  Refusals as for the other shades, and n_records beyond 2^31 - 1 (it
 * needs no materials). */
int trx_material_compose_dev(trx_scene *scene, const trx_hit *d_primary, const float *d_direct, const float *d_indirect_rgb,
                             uint64_t n_records, float *d_colour_rgb, void *stream);
int trx_shade_rgb_dev(trx_scene *scene, const float *d_colour_rgb, uint64_t n_records, uint8_t *d_rgba, void *stream);

/* trx_render_image_gi_sparse in colour (synchronous): the lit chain up to the light term V; with bounce_samples == 0 the
 * compose without an indirect term; otherwise the RGB indirect pass - trx_trace_indirect_rgb_dev at bounce_stride 1,
 * trx_trace_indirect_rgb_sparse_dev (bounce_stride, bounce_phase) above it - then per plane trx_value_upsample_dev without a
 * base when bounce_stride > 1 and trx_value_filter_dev without a base when bounce_filter_levels >= 1; then
 * trx_material_compose_dev with V and trx_shade_rgb_dev; 4 bytes per pixel are copied back (out_rgba may be NULL).
 * bounce_stride is 1..TRX_MAX_AO_STRIDE; the tolerances are looked at when a step uses them.  Every argument is validated
 * before the first pass is enqueued; refused on a scene without materials. */
int trx_render_image_colour(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                            uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                            uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                            float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos,
                            uint32_t bounce_samples, float bounce_eps, uint32_t bounce_filter_levels, float bounce_depth_tol,
                            float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase,
                            uint32_t bounce_upsample_radius, uint8_t *out_rgba, float *out_ms);

/* Materials of the generated scenes (trx_gen_scene), for the mesh as generated: verts (n_tris x 9 floats) and object_counts
 * (n_objects triangle counts) as trx_gen_scene returned them.  *out_materials (n entries at *out_n_materials) and
 * *out_tri_material (n_tris indices, in the order of verts) are trx_free'd by the caller.
 *  "cornell": material 0 albedo (0.8, 0.8, 0.8); material 1 albedo (0.8, 0, 0) for every triangle whose three x are all
 *  exactly -1.0f (the left wall); material 2 albedo (0, 0.8, 0) for all x exactly +1.0f (the right wall); material 3 albedo 0,
 *  emission (4, 4, 4) for the triangles of the last object (the light quad); material 0 for the rest.
 *  Any other name: six materials, emission 0, albedo palette = {(.8,.8,.8), (.8,.4,.3), (.3,.6,.8), (.5,.7,.3), (.8,.7,.4),
 *  (.6,.5,.7)}; every triangle of object j gets material j % 6.
 * Refused (TRX_ERR_INVALID): null arguments, object counts that do not sum to n_tris. */
int trx_standin_materials(const char *name, const float *verts, uint64_t n_tris, const uint64_t *object_counts,
                          uint32_t n_objects, trx_material **out_materials, uint32_t *out_n_materials,
                          uint16_t **out_tri_material);

/* trx_load_model with the model's materials: the same verts and object counts, byte for byte, plus a material table and
 * tri_material in that triangle order (all four trx_free'd by the caller).  Material 0 always exists and is the default: albedo
 * (0.8, 0.8, 0.8), emission 0.  OBJ: every `mtllib` file is read from the OBJ's directory; its `newmtl` entries follow in file
 * order; `Kd` gives the albedo (a missing Kd: 0.8 each), `Ke` the emission (a missing Ke: 0); nothing else of a material is
 * read.  `usemtl` names are looked up once the whole OBJ is read (the first material of a name wins).  Material 0 goes to:
 * faces before any usemtl, an unknown name, everything when the mtl file is missing, every triangle of a JSON model.  A
 * quad's two triangles share a material.  Refused with TRX_ERR_INVALID: a negative or non-finite Kd or Ke (or one that is not
 * three numbers), more than 65535 named materials, null arguments; TRX_ERR_IO: an unreadable model, as trx_load_model. */
int trx_load_model_materials(const char *path, float **out_verts, uint64_t *out_n_tris, uint64_t **out_object_counts,
                             uint32_t *out_n_objects, trx_material **out_materials, uint32_t *out_n_materials,
                             uint16_t **out_tri_material);

/* ---- emitters: emissive triangles sampled as lights at primary and bounce hits ---------------------------------------------------
 * Above, an emissive triangle lights the scene only when a cosine-distributed bounce ray happens to hit it.  This section
 * samples the emitters directly (next-event estimation): a device-built table of the scene's emissive triangles, a pass that
 * casts one shadow ray per sample toward a point on a selected emitter from every primary hit, and a mode of the RGB indirect
 * pass that does the same from every bounce hit.  Purely additive: every call above computes what it computed.
 *
 * THE EMITTER TABLE.  An emitter is one (instance, triangle) pair whose material has any emission component > 0.  On a
 * single-level scene the emitters are the emissive triangles in `prim` order (instance id 0xFFFFFFFF); on a two-level scene
 * every TLAS primitive k, ascending, crossed with the emissive triangles reachable from its entry node (its BLAS), ascending
 * by `prim`.  trx_scene_build_emitters needs materials, finds the pairs on the host and refuses with TRX_ERR_INVALID when there
 * are none or more than TRX_MAX_EMITTERS; *out_n (may be NULL) receives the count.  The device then writes one 64-byte record
 * per emitter from the scene's own 48-byte triangle records {v0, e1, e2, cross(e1, e2)}.  That record stores e1 = v0 - v1
 * (and e2 = v2 - v0), so the emitter's first edge is E1 = -e1 (the sign flipped, nothing rounded) = v1 - v0 and E2 = e2:
 * V0 + b1 * E1 + b2 * E2 with b1, b2 >= 0, b1 + b2 <= 1 lies in the triangle.  Where the scene has instance transforms, with
 * m the instance's object-to-world matrix as trx_scene_set_instance_transforms took it (m[c * 4 + r]), a point p becomes
 *   P_r = ((m[r] * p.x + m[4 + r] * p.y) + m[8 + r] * p.z) + m[12 + r]
 * and an edge e becomes (m[r] * e.x + m[4 + r] * e.y) + m[8 + r] * e.z, r = 0, 1, 2: every operation rounded once in binary32,
 * no contraction; without transforms the record's values are taken as they are.  NG = cross(E1, E2) of the world-space
 * edges: NG.x = E1.y * E2.z - E1.z * E2.y and cyclic, two products and one subtraction, each rounded once.
 *   record (16 floats): V0.x V0.y V0.z kinv | E1.x E1.y E1.z material | E2.x E2.y E2.z prim | NG.x NG.y NG.z instance
 *   (material, prim, instance: the uint32 as the bit pattern of the float lane).
 * The host reads the records back and builds the selection table in binary64, in index order, with Le = the emission of the
 * record's material:  w_j = sqrt(NG.x^2 + NG.y^2 + NG.z^2) * (Le_r + Le_g + Le_b),  W = sum of w_j,
 *   p_j = 0.5 * w_j / W + 0.5 / n   (p_j = 1 / n when W == 0),
 *   P_j = (float)p_j,  kinv_j = (float)(1.0 / (3.14159265358979323846 * (double)P_j)),
 *   c_i = (float)(p_0 + ... + p_i) for i = 0 .. n - 2 (a dense array; none for n == 1).
 * The defensive half keeps every p_j >= 0.5 / n: no weight can overflow, a zero-area emitter is harmless.
 * SELECTION for u0 in [0, 1]: j = the number of i in 0 .. n - 2 with c_i <= u0.  The device finds it by bisection (at most 20
 * steps); there is no clamp, no special case for u0 == 1.0f (which the hash does produce) and none for n == 1.
 * Ownership is that of the material tables: counted by trx_scene_device_bytes (64 B per emitter and 4 B per c_i, at least one),
 * released by trx_scene_destroy, replaced by a second build under the launch mutex after the scene's launches in flight.
 * STALENESS.  The table holds world-space geometry and material indices: a later trx_scene_set_materials, trx_scene_refit*,
 * trx_scene_set_instance_transforms or trx_scene_set_instance_entry_nodes marks it stale, and every emitter entry point then
 * refuses with TRX_ERR_INVALID until trx_scene_build_emitters has run again (a flag on the host; no kernel of those calls changed).
 * trx_scene_get_emitters: *inout_n holds the capacity of out_records in emitters on entry (out_c then has room for capacity - 1
 * floats) and the table's size on return; refused without a table, with a stale one, or with too little room. */
#define TRX_MAX_EMITTERS (1u << 20)
int trx_scene_build_emitters(trx_scene *scene, uint32_t *out_n);
int trx_scene_get_emitters(const trx_scene *scene, float *out_records, uint32_t *inout_n, float *out_c);

/* THE EMITTER LIGHT PASS at primary hits.  For pixel (px, py) and sample f in 0 .. n_samples - 1 (n_samples in
 * 1..TRX_MAX_AO_SAMPLES); every operation rounded once in binary32, no contraction; dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *  E1. Surface pixel, flipped unit normal n and origin o are THE SHADOW RAY's statements with shadow_eps - the caller-record
 *      rule and the required d_primary_inst on a scene with instance transforms included.  Any other pixel gets the inert ray.
 *  E2. se = frame0 + 2048u + f;  u0 = hash_noise(px, py, se), u1 = hash_noise(px, py, se + 1024u),
 *      u2 = hash_noise(px, py, se + 4096u).  (AO and bounce rays use frame0 + f and + 1024; rect lights stay below frame0 + 1600.)
 *  E3. j is selected by u0.  su = sqrtf(u1), b1 = su * (1.0f - u2), b2 = su * u2, y[i] = (V0[i] + b1 * E1[i]) + b2 * E2[i].
 *  E4. v = y - o, q = dot3(v, v), dist = sqrtf(q), inv = 1.0f / dist, l = v * inv; tmin = 0, tmax = dist - dist * emitter_eps
 *      (emitter_eps finite, in [0, 1): it stops the ray short of the emitter's own triangle); c = dot3(n, l),
 *      a = 0.5f * fabsf(dot3(NG, l)) (emission is two-sided, as in rule 5c; cos x area needs no normalisation),
 *      wgeo = ((c * a) / q) * kinv_j.  The ray is CAST iff c > 0.0f && wgeo > 0.0f && wgeo < +inf; otherwise the sample gets
 *      the inert ray and contributes nothing (NaN, a light at the hit point, a zero-area or edge-on emitter).
 *  E5. A_c = 0.0f; for f ascending, if the ray was cast and is NOT occluded (trx_trace_occluded_dev's answer, or
 *      trx_trace_occluded_masked_dev's with ray_mask 1..255): A_c = A_c + wgeo_f * emission_c(material of emitter j_f).
 *      out_c = base_c + A_c / (float)n_samples at a surface record, base_c elsewhere; base_c = d_base_rgb[c * records + r], +0.0f
 *      with d_base_rgb == NULL.  d_base_rgb may be d_out_rgb: each lane reads before it writes.  A record outside the shard or
 *      the image is untouched.  The order holds under any scratch cap.
 * The 1 / pi inside kinv makes the pass estimate what rule 5c's "+ emission_c(m)" term estimates over cosine-distributed bounce
 * rays: the mean of emission_c over the hemisphere, cosine-weighted.
 * trx_emitter_rays_dev writes one sample's rays, one per record of `shard`, like trx_light_rays_dev (sample in
 * 0..TRX_MAX_AO_SAMPLES - 1).  trx_trace_emitter_light_dev is the pass: three planes at c * records by
 * trx_trace_light_visibility_dev's plane rule; its mechanics too - the stream's launch slot, [tile][sample][64] scratch under
 * the same cap, no host synchronisation.  Refused with TRX_ERR_INVALID before anything is enqueued (the output left as it
 * was): a null scene, d_primary or output, n_samples or sample out of range, unknown semantics bits, ray_mask > 255, a
 * negative or NaN shadow_eps, an emitter_eps outside [0, 1), a missing d_primary_inst on a transformed scene, a scene without
 * an emitter table or with a stale one. */
int trx_emitter_rays_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                         uint32_t frame0, uint32_t sample, float shadow_eps, float emitter_eps, const trx_hit *d_primary,
                         const uint32_t *d_primary_inst, trx_ray *d_rays, void *stream);
int trx_trace_emitter_light_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                                uint32_t semantics, uint32_t ray_mask, uint32_t frame0, uint32_t n_samples, float shadow_eps,
                                float emitter_eps, const trx_hit *d_primary, const uint32_t *d_primary_inst,
                                const float *d_base_rgb, float *d_out_rgb, void *stream);

/* EMITTERS AT BOUNCE HITS.  trx_trace_indirect_rgb_dev with one more argument, emitter_eps; n_lights may be 0 (lights may
 * then be NULL).  Rules 1 to 4 are unchanged - bounce ray, bounce hit, the lights' shadow rays and s_f are bit for bit the
 * existing pass's; with 0 lights s_f = +0.0f.  For every bounce with a surface, rules E2 to E4 then apply with the primary hit
 * replaced by the bounce hit: d is the bounce ray's direction, n the flipped attr.normal of rule 3, o[i] = Q[i] - d[i] *
 * shadow_eps, the seed se = frame0 + 8192u + f hashed at the pixel of the full-resolution image (as the rect noise is); the
 * any-hit launch is masked when ray_mask != 0.  In rule 5c's place:
 *  5e. For f ascending, where bounce f has a surface: m = tri_material[bounce_hit_f.prim], X_c = wgeo_f * emission_c(emitter
 *      j_f) if that ray was cast and is not occluded, else +0.0f, and A_c = A_c + albedo_c(m) * (s_f + X_c) - the inner
 *      addition, then the product, then the outer addition.  There is no "+ emission_c(m)" term: light that reaches the
 *      primary hit straight from an emitter belongs to trx_trace_emitter_light_dev, and counting it here too would count it
 *      twice.  out_c = A_c / (float)n_samples.
 * The sparse form is trx_trace_indirect_rgb_sparse_dev's statement: each cell is bit for bit the dense value of its pixel.
 * Refusals: everything trx_trace_indirect_rgb_dev refuses except n_lights == 0, and what the emitter pass refuses of
 * emitter_eps and the table. */
int trx_trace_indirect_rgb_emitters_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                        trx_shard shard, uint32_t semantics, uint32_t ray_mask, const trx_light *lights,
                                        uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float bounce_eps,
                                        float shadow_eps, float emitter_eps, const trx_hit *d_primary,
                                        const uint32_t *d_primary_inst, float *d_value_rgb, void *stream);
int trx_trace_indirect_rgb_emitters_sparse_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                               uint32_t stride, uint32_t phase, uint32_t semantics, uint32_t ray_mask,
                                               const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                               uint32_t n_samples, float bounce_eps, float shadow_eps, float emitter_eps,
                                               const trx_hit *d_primary, const uint32_t *d_primary_inst,
                                               float *d_value_rgb_lo, void *stream);

/* trx_render_image_colour with the emitters sampled (synchronous): trx_render_image_colour's arguments plus emitter_samples
 * (1..TRX_MAX_AO_SAMPLES) and emitter_eps; n_lights may be 0.  The chain: the lit chain up to V - with no lights V is the
 * AO-scaled ambient alone, what trx_light_term_dev gives for one light of intensity 0; with bounce_samples >= 1 the
 * emitter-mode indirect pass, dense or sparse, then upsample and filter per plane as in trx_render_image_colour; then
 * trx_trace_emitter_light_dev at full resolution, dense and unfiltered (direct shadows stay sharp), with the filtered planes
 * as both base and output (no base with bounce_samples == 0); then trx_material_compose_dev and trx_shade_rgb_dev.  It builds
 * the emitter table first if the scene has none, or a stale one. */
int trx_render_image_colour_emitters(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                     uint32_t semantics, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                                     uint32_t frame0, uint32_t light_samples, float shadow_eps, float ambient,
                                     uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                                     float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t bounce_filter_levels,
                                     float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride,
                                     uint32_t bounce_phase, uint32_t bounce_upsample_radius, uint32_t emitter_samples,
                                     float emitter_eps, uint8_t *out_rgba, float *out_ms);

/* Counting variant (PROFILE_RT): same traversal, also accumulates trx_stats.
 * Synchronous; d_hits may be NULL.  trx_count_ao: d_primary may hold any bit pattern - a record that is no surface record
 * of this scene is a miss, no ray and nothing counted (CALLER RECORDS, above). */
int trx_count_primary(trx_scene *scene, const trx_view *view, uint32_t width,
                      uint32_t height, trx_shard shard, uint32_t semantics,
                      trx_hit *d_hits, trx_stats *stats);
int trx_count_ao(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                 trx_shard shard, uint32_t semantics, uint32_t frame, float ao_eps,
                 const trx_hit *d_primary, trx_hit *d_ao, trx_stats *stats);
int trx_count_rays(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays,
                   uint32_t semantics, trx_hit *d_hits, trx_stats *stats);

/* Per-ray counts of a counting pass: every ray's own share of trx_stats.n_node and trx_stats.n_tri.
 *   n_node  node visits of this ray (the reference's aabb_hit_count / 8); on a two-level scene both levels count
 *   n_tri   triangle tests of this ray (the reference's tri_hit_count)
 * each saturated at 65535.  The sums of the records a pass writes are its trx_stats.n_node / n_tri (short of saturation).
 * The three calls are trx_count_primary / trx_count_ao / trx_count_rays - same arguments, same per-scene lock, same
 * synchronous protocol on the null stream, same trx_stats and hit records - with one more output: d_cost, device memory
 * indexed exactly like the hit buffer of the call (both layouts, any shard).  Records of other shards, of pixels outside
 * the image and past the end of the buffer are left as they were; an AO pixel whose primary record is a miss gets {0, 0}.
 * d_hits / d_ao may be NULL (the records go to the scene's scratch).  A null d_cost is refused with TRX_ERR_INVALID before
 * anything is enqueued.  Counting passes are never timed; fused frames and the ray service have no per-ray counts. */
typedef struct trx_ray_cost {
    uint16_t n_node;
    uint16_t n_tri;
} trx_ray_cost; /* 4 bytes */
/* (trx_count_ao_per_ray: d_primary may hold any bit pattern - a record that is no surface record of this scene is a miss and
 * gets {0, 0}: CALLER RECORDS, above.) */
int trx_count_primary_per_ray(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                              uint32_t semantics, trx_hit *d_hits, trx_ray_cost *d_cost, trx_stats *stats);
int trx_count_ao_per_ray(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                         uint32_t semantics, uint32_t frame, float ao_eps, const trx_hit *d_primary, trx_hit *d_ao,
                         trx_ray_cost *d_cost, trx_stats *stats);
int trx_count_rays_per_ray(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, uint32_t semantics, trx_hit *d_hits,
                           trx_ray_cost *d_cost, trx_stats *stats);

/* The PROFILE_RT heat map (the reference's profiling build of its pixel program, rt_gpu_software.hlsl:84-102): a colour
 * per record from its per-ray counts.  Elementwise over n_records records in ANY layout, like the shades above: 4 bytes
 * {r, g, b, 255} per record at d_rgba (n_records * 4 bytes, 4-byte aligned; nothing beyond them is written).
 *   TRX_HEAT_NODES  x = (float)(8 * n_node) * scale   (the reference: aabb_hit_count * 0.002)
 *   TRX_HEAT_TRIS   x = (float)n_tri * scale          (the reference's commented-out alternative: tri_hit_count * 0.01)
 * The colour of x is the reference's `temperature` (sampling.hlsl:54-83) as a rule; every operation in binary32, rounded
 * once, no contraction, the division an IEEE division:
 *   s = x * 10;  cur = min((int)s, 9) (truncation);  prv = max(cur - 1, 0);  nxt = min(cur + 1, 9);
 *   S(a, b, v): q = clamp((v - a) / (b - a), 0, 1), result (q * q) * (3 - 2 * q);
 *   c = (float)cur;  lo = S(c - 0.8f, c + 0.8f, s);  hi = S((c + 1) - 0.8f, (c + 1) + 0.8f, s);
 *   wc = lo * (1 - hi);  wp = 1 - lo;  wn = hi;
 *   per channel r = (wc * P[cur] + wp * P[prv]) + wn * P[nxt], clamped to [0, 1], with the ten palette rows P = k / 255.0f,
 *   k = (0,2,91) (0,108,251) (0,221,221) (51,221,0) (255,252,0) (255,180,0) (255,104,0) (226,22,0) (191,0,83) (145,0,65);
 *   the byte is (uint8_t)floorf(r * 255.0f + 0.5f) (the unorm8 store of an rgba8 target); alpha is 255.
 * No pow is applied (the reference's pow(col, 2.2) belongs to its other branch).  At the reference scales the image is
 * constant from n_node = 61 (61 distinct colours) and from n_tri = 98 (97 distinct colours) on.
 * Refused with TRX_ERR_INVALID before anything is enqueued, the output untouched: a null scene or - with n_records != 0 - a
 * null buffer, a misaligned d_rgba, which > 1, a scale that is NaN, negative or infinite.  n_records == 0 does nothing. */
#define TRX_HEAT_NODES 0u
#define TRX_HEAT_TRIS 1u
#define TRX_HEAT_SCALE_NODES 0.002f
#define TRX_HEAT_SCALE_TRIS 0.01f
int trx_shade_heat_dev(trx_scene *scene, const trx_ray_cost *d_cost, uint64_t n_records, uint32_t which, float scale,
                       uint8_t *d_rgba, void *stream);
/* Host-buffer form for a whole image (synchronous, under the per-scene lock): the counted primary pass and the heat shade;
 * only the width * height * 4 bytes of out_rgba (may be NULL) cross the bus; out_stats (may be NULL) takes the pass's
 * trx_stats.  Every argument is validated before the first pass. */
int trx_render_heat_image(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                          uint32_t which, float scale, uint8_t *out_rgba, trx_stats *out_stats);

/* ---- vertex normals and the shading normal: smooth normals for the light term and the edge-aware filters ---------------------------
 * Every pass above shades with the geometric normal of the committed triangle (trx_hit_attr.normal), so a tessellated curved
 * surface comes out faceted and its facet edges fail the filters' normal test in the middle of a smooth surface.  This section
 * gives a scene a table of vertex normals keyed by trx_hit.prim and a pass that rewrites the normal of attribute records from
 * it; trx_light_term_dev, trx_ao_filter_dev, trx_ao_upsample_dev, trx_value_filter_dev and trx_value_upsample_dev take the
 * rewritten buffer as they take any attribute buffer.  Purely additive: every call above computes what it computed.  Ray
 * origins, bounce directions and the facing of shadow rays stay geometric - every ray-generating pass derives its normal from
 * the triangle itself - which is what keeps an offset origin on the lit side of its own triangle.
 *
 * THE TABLE.  normals holds nine floats per triangle: the object-space normals of vertices 0, 1 and 2 of triangle i of the
 * buffer handed to trx_scene_create - `prim` order; a caller with a trx_flat applies tri_source, as for tri_material.  On a
 * two-level scene the instances of a BLAS share its triangles' normals.  trx_scene_set_vertex_normals validates on the host
 * before anything is copied and refuses with TRX_ERR_INVALID: n_tris different from the scene's, any component that is not
 * finite.  Zero and unnormalised vectors are legal: the rule below handles them.  normals == NULL or n_tris == 0 removes the
 * table.  On the device the table is three float4 per triangle (w = +0).  It is owned like the material table: counted by
 * trx_scene_device_bytes at 48 B per triangle, released by trx_scene_destroy; a second call replaces it after waiting for the
 * scene's launches in flight, which see the old table in full; a refused call leaves the old table in force.  A refit KEEPS
 * the table as it is: a caller whose refit changed the shape of the mesh sets the normals again.
 * trx_scene_get_vertex_normals returns the caller's floats bit for bit; refused on a scene without a table or with n_tris
 * different from the scene's. */
int trx_scene_set_vertex_normals(trx_scene *scene, const float *normals, uint64_t n_tris);
int trx_scene_get_vertex_normals(const trx_scene *scene, float *out_normals, uint64_t n_tris);

/* THE SHADING NORMAL of a record.  Every operation is rounded once in binary32, no contraction;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  In: the record's hit (t, prim), its instance id on a scene with instance
 * transforms, its trx_hit_attr A - u, v and the world unit geometric normal g = A.normal - and the world ray direction d:
 * primary_dir of the pixel as given (the primary form), or the ray's direction words as stored (the rays form); no
 * zero-direction fix is applied, as in the light term.
 *  N1. A record with prim >= n_tris, or with an instance id >= n_instances on a scene with instance transforms, is out of
 *      range: it reads no table and out = A bit for bit (CALLER RECORDS, above; t is not looked at, as in the attribute pass).
 *  N2. Otherwise, with n0, n1, n2 the triangle's vertex normals: w = (1.0f - u) - v and, per component c,
 *      m[c] = (w*n0[c] + u*n1[c]) + v*n2[c].  On a scene with instance transforms m goes to world space exactly as the
 *      attribute pass takes the geometric normal there: with r0, r1, r2 the instance's world-to-object rows,
 *      m' = ((r0.x*m.x + r1.x*m.y) + r2.x*m.z, (r0.y*m.x + r1.y*m.y) + r2.y*m.z, (r0.z*m.x + r1.z*m.y) + r2.z*m.z).
 *  N3. q = dot3(m, m);  s = m * (1.0f / sqrtf(q)) (an IEEE square root, an IEEE division, three multiplications);
 *      c = dot3(s, g);  s = s * copysignf(1.0f, c).
 *  N4. a = (g.x*-d.x + g.y*-d.y) + g.z*-d.z and b = (s.x*-d.x + s.y*-d.y) + s.z*-d.z - the light term's argument of its flip.
 *  N5. The record is ADOPTED iff q > 0.0f and q < +inf and c == c and ((a > 0.0f and b > 0.0f) or (a < 0.0f and b < 0.0f)).
 *      An adopted record gets out = {A.u, A.v, s, _pad = 0}; any other record gets out = A bit for bit.
 * What N5's last condition buys: the light term's flip copysignf(1, .) is the same for s as for g, so a smooth normal never
 * lights the back of a silhouette triangle.  Zero, NaN-producing and overflowing vertex normals fall back to the geometric
 * normal, and so does a record whose A carries a NaN.
 * Layouts and untouched records are those of trx_hit_attributes_*_dev: the primary form takes d_hits / d_inst / d_attr /
 * d_out laid out by `shard`; in image layout the records of pixels outside the shard are left untouched, and so are a compact
 * tile's pixels outside the image.  d_out may be d_attr: each lane reads its record before it writes it.  The rays form
 * reads the direction words of d_rays alone.  Refused with TRX_ERR_INVALID before anything is enqueued, the output left as it
 * was: a scene without a vertex-normal table, a null buffer, a missing d_inst on a scene with instance transforms, everything
 * the attribute calls refuse of image and shard.  The launches take a launch slot as the attribute pass does: a refit or a
 * table swap called afterwards waits for the pass, which sees the old tables in full. */
int trx_shading_normals_primary_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                                    const trx_hit *d_hits, const uint32_t *d_inst, const trx_hit_attr *d_attr,
                                    trx_hit_attr *d_out, void *stream);
int trx_shading_normals_rays_dev(trx_scene *scene, const trx_ray *d_rays, uint64_t n_rays, const trx_hit *d_hits,
                                 const uint32_t *d_inst, const trx_hit_attr *d_attr, trx_hit_attr *d_out, void *stream);

/* trx_render_image_lit and trx_render_image_colour with the shading-normal pass inserted right after the attribute pass
 * (synchronous): the shading attributes take the attribute buffer's place in the light term and in every filter and upsample
 * call; every ray-generating pass keeps its own geometric normals.  Arguments, validation and order are the plain forms';
 * refused in addition on a scene without a vertex-normal table.  With an all-zero table every record falls back and the image
 * is the plain form's byte for byte. */
int trx_render_image_lit_smooth(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                                uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                                float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos, uint8_t *out_rgba,
                                float *out_ms);
int trx_render_image_colour_smooth(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                   uint32_t semantics, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                                   uint32_t frame0, uint32_t light_samples, float shadow_eps, float ambient,
                                   uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                                   float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t bounce_filter_levels,
                                   float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride,
                                   uint32_t bounce_phase, uint32_t bounce_upsample_radius, uint8_t *out_rgba, float *out_ms);

/* Vertex normals from the mesh alone (host): verts holds n_tris x 9 floats, out_normals receives n_tris x 9.  Every operation
 * in binary64, rounded once, no contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  The face vector of a triangle is
 * F = cross(v1 - v0, v2 - v0), its unit face vector F / sqrt(dot(F, F)) per component.  A face whose sqrt(dot(F, F)) is zero or
 * not finite contributes nowhere and its own corners get +0 (which THE SHADING NORMAL turns into the geometric normal).  For
 * every other corner, S = the sum, in ascending triangle index, of the face vectors F of this triangle and of every other
 * contributing triangle that has a corner at the bitwise-same position (-0.0 taken as +0.0) and whose unit face vector has a
 * dot product >= crease_cos with this triangle's; the corner gets (float)(S[c] / sqrt(dot(S, S))), or +0 when that square
 * root is zero or not finite.  The weights are the faces' areas.  Welding is over the whole buffer.  crease_cos = 1 gives
 * flat normals up to coplanar neighbours, -1 welds everything.  Refused (TRX_ERR_INVALID): null arguments, crease_cos
 * outside [-1, 1] or NaN, more than 2^32 / 3 triangles. */
int trx_compute_vertex_normals(const float *verts, uint64_t n_tris, float crease_cos, float *out_normals);

/* trx_load_model with the model's vertex normals: the same verts and object counts, byte for byte, plus nine floats per
 * triangle in that triangle order (all trx_free'd by the caller).  OBJ: `vn` records are read; the third index of a face
 * corner's v/vt/vn or v//vn names one, relative to the `vn` records read so far when negative.  A corner with no normal index,
 * or with one out of range at that point of the file, gets +0.  A quad's two triangles take corners 0,1,2 and 0,2,3, as for
 * positions.  A JSON model gets +0 everywhere.  *out_has_normals is 1 when any corner got a `vn`, else 0.  Refused with
 * TRX_ERR_INVALID: a `vn` with a component that is not finite, null arguments; TRX_ERR_IO: an unreadable model. */
int trx_load_model_normals(const char *path, float **out_verts, uint64_t *out_n_tris, uint64_t **out_object_counts,
                           uint32_t *out_n_objects, float **out_normals, uint32_t *out_has_normals);

/* ---- texture coordinates and albedo textures: the surface's colour from an image ------------------------------------------------------
 * Above, a triangle's albedo is its material's, flat.  This section gives a scene a table of texture coordinates keyed by
 * trx_hit.prim, a set of RGBA8 textures keyed by material, a pass that writes the albedo of every hit record - the material's,
 * times the texture sampled at the hit's interpolated coordinates - and a compose that reads that albedo in place of the
 * material's.  Purely additive: every call above computes what it computed, with or without these tables on the scene.
 *
 * THE TEXCOORD TABLE.  uvs holds six floats per triangle, (s0, t0, s1, t1, s2, t2): the coordinates of vertices 0, 1 and 2 of
 * triangle i of the scene's own order - the `prim` a hit record carries.  They are object-space: the instances of a BLAS share
 * them, and neither a view nor an instance id is needed to use them.  Any float is legal, non-finite ones included: THE TEXTURED
 * ALBEDO below handles them.  uvs == NULL or n_tris == 0 removes the table.  24 B per triangle on the device, counted by
 * trx_scene_device_bytes.  Owned exactly like the vertex normals: the swap waits for every launch slot's last kernel, so a pass
 * enqueued before the call uses the old table in full; trx_scene_refit keeps the table; it goes with the scene.
 * trx_scene_get_texcoords returns the caller's floats bit for bit.  Refused (TRX_ERR_INVALID): a null scene, n_tris different
 * from the scene's; the getter also on a scene without a table, and with a null output. */
int trx_scene_set_texcoords(trx_scene *scene, const float *uvs, uint64_t n_tris);
int trx_scene_get_texcoords(const trx_scene *scene, float *out_uvs, uint64_t n_tris);

/* THE TEXTURE SET.  descs names n_textures textures; texels is one array of n_texels RGBA8 words (R in the low byte, then G, B,
 * A), the textures back to back in descriptor order, each row-major, row 0 being the row at t = 0 (a loader of top-down image
 * files flips the rows).  material_texture[m] is the texture of material m, or TRX_NO_TEXTURE.  Everything is validated on the
 * host before anything is copied, so that no kernel needs a bound on an index (as with tri_material).  Refused
 * (TRX_ERR_INVALID), the old set left in force: null arguments; a scene without materials; n_materials different from the
 * scene's; an index >= n_textures that is not TRX_NO_TEXTURE; a width or height outside 1..TRX_MAX_TEXTURE_SIZE; n_textures
 * outside 1..TRX_MAX_TEXTURES; n_texels different from the sum of width * height, or >= 2^31; an unknown format or filter.
 * On the device: a 16-byte descriptor per texture {offset of its first texel, width, height, format | filter << 8}, the texel
 * words, the per-material index and the 256 floats of trx_texture_srgb_table - all counted by trx_scene_device_bytes.  Owned
 * like the materials (swap under the launch mutex, the old set freed after every launch slot's last kernel, kept by a refit).
 * The set is keyed by material: a later trx_scene_set_materials with a different n_materials drops it (one with the same
 * count keeps it).  trx_scene_remove_textures drops it.  trx_scene_get_textures returns what was set, bit for bit:
 * *inout_n_textures, *inout_n_texels and *inout_n_materials hold the capacities of the three arrays on entry and the counts on
 * return; refused on a scene without a set, with null arguments or with too little room (the counts are still returned). */
typedef struct trx_texture_desc {
    uint32_t width, height;
    uint32_t format; /* TRX_TEX_RGBA8_UNORM / TRX_TEX_RGBA8_SRGB */
    uint32_t filter; /* TRX_TEX_NEAREST / TRX_TEX_BILINEAR */
} trx_texture_desc;
#define TRX_TEX_RGBA8_UNORM 0u
#define TRX_TEX_RGBA8_SRGB 1u
#define TRX_TEX_NEAREST 0u
#define TRX_TEX_BILINEAR 1u
#define TRX_NO_TEXTURE 0xFFFFFFFFu
#define TRX_MAX_TEXTURE_SIZE 8192u
#define TRX_MAX_TEXTURES 65535u
int trx_scene_set_textures(trx_scene *scene, const trx_texture_desc *descs, uint32_t n_textures, const uint32_t *texels,
                           uint64_t n_texels, const uint32_t *material_texture, uint32_t n_materials);
int trx_scene_get_textures(const trx_scene *scene, trx_texture_desc *out_descs, uint32_t *inout_n_textures, uint32_t *out_texels,
                           uint64_t *inout_n_texels, uint32_t *out_material_texture, uint32_t *inout_n_materials);
int trx_scene_remove_textures(trx_scene *scene);

/* The sRGB decode table: out[c] for c = 0..255, with x = c / 255 in binary64, is x / 12.92 for x <= 0.04045 and
 * pow((x + 0.055) / 1.055, 2.4) otherwise, computed in binary64 and rounded once to float. */
void trx_texture_srgb_table(float out[256]);

/* THE TEXTURED ALBEDO.  Every operation is rounded once in binary32, no contraction.
 *  Which records.  A record is a surface record if t < FLT_MAX, prim != 0xFFFFFFFF and prim < n_tris.  Any other record is
 *  background: +0.0f in all three planes.  For a surface record m = tri_material[prim], T = material_texture[m], and
 *  A_c = albedo_c(m) exactly when the scene has no texcoord table, no texture set, or T is TRX_NO_TEXTURE.
 *  Interpolation and wrap.  Otherwise, with u, v of the record's trx_hit_attr and (s0, t0, s1, t1, s2, t2) of triangle prim:
 *  w = (1.0f - u) - v, s = (w * s0 + u * s1) + v * s2 and t = (w * t0 + u * t1) + v * t2 (the association of THE SHADING
 *  NORMAL).  If s or t is not finite, A_c = albedo_c(m).  The wrap is repeat: fs = s - floorf(s); if fs >= 1.0f (a tiny
 *  negative s, whose subtraction rounds to 1) fs = 0.0f.  ft likewise from t.  W, H = the texture's width and height.
 *  Nearest.  ix = min((uint32_t)(fs * (float)W), W - 1), iy = min((uint32_t)(ft * (float)H), H - 1); one tap, val_c its channel.
 *  Bilinear.  x = fs * (float)W - 0.5f, x0 = floorf(x), fx = x - x0, ix0 = (int)x0, ix1 = ix0 + 1; ix0 == -1 becomes W - 1 and
 *  ix1 == W becomes 0.  y, y0, fy, iy0, iy1 the same from ft and H.  With c00 = the channel of tap (ix0, iy0), c10 of
 *  (ix1, iy0), c01 of (ix0, iy1), c11 of (ix1, iy1): top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01),
 *  val_c = top + fy * (bot - top).
 *  Texel decode.  Tap (ix, iy) is word offset + iy * W + ix of the texel array; its channel byte c8 (R bits 0..7, G 8..15,
 *  B 16..23) decodes as (float)c8 / 255.0f (one IEEE division) for TRX_TEX_RGBA8_UNORM and as trx_texture_srgb_table's entry
 *  c8 for TRX_TEX_RGBA8_SRGB.  Alpha is read and ignored.
 *  The albedo.  A_c = albedo_c(m) * val_c.
 * trx_surface_albedo_dev writes A_c of n_records records in any layout - d_hits and d_attr as a trace and its attribute pass
 * (or a caller) wrote them; it is elementwise - into three planes, plane c at c * n_records.  u and v are used as they are,
 * whatever they hold (CALLER RECORDS, above: a record whose prim is no triangle of the scene is background, every index formed
 * from a record stays inside its table).  It takes a launch slot as the attribute pass does: a table swap or a refit called
 * afterwards waits for it.  Texcoords and textures are optional: without them it writes the plain albedo.  Refused
 * (TRX_ERR_INVALID): null arguments, n_records == 0 or beyond 2^31 - 1, a scene without materials. */
int trx_surface_albedo_dev(trx_scene *scene, const trx_hit *d_hits, const trx_hit_attr *d_attr, uint64_t n_records,
                           float *d_albedo_rgb, void *stream);

/* trx_material_compose_dev with albedo_c(m) read from an albedo plane: for a surface record (the same rule)
 * colour_c = emission_c(m) + A_c * (E + I_c), A_c = d_albedo_rgb[c * n_records + r] - the same association, each operation
 * rounded once; emission_c(m) + A_c * E with d_indirect_rgb == NULL; +0.0f in all three planes for any other record.
 * d_colour_rgb may be d_indirect_rgb: each lane reads before it writes.  On planes trx_surface_albedo_dev wrote for a scene
 * without a texture set this is trx_material_compose_dev bit for bit.  Refusals as trx_material_compose_dev, plus a null
 * albedo plane. */
int trx_albedo_compose_dev(trx_scene *scene, const trx_hit *d_primary, const float *d_albedo_rgb, const float *d_direct,
                           const float *d_indirect_rgb, uint64_t n_records, float *d_colour_rgb, void *stream);

/* THE TEXTURED RGB INDIRECT TERM.  One entry point for the four RGB modes of the indirect pass, with albedo_c(m) of rules 5c
 * and 5e replaced by A_c of THE TEXTURED ALBEDO sampled at the bounce hit: prim = bounce_hit_f.prim, u and v those of the
 * bounce hit's attribute record (what trx_hit_attributes_rays_dev writes for the bounce ray, its hit and its instance id).
 * The rules are otherwise word for word: 5c is A_c = A_c + (A_c(bounce f) * s_f + emission_c(m)), 5e is
 * A_c = A_c + A_c(bounce f) * (s_f + X_c).  Bounce rays, hits, shadow rays, s_f, wgeo and the selected emitters are the
 * existing passes' bit for bit; only the gather differs, and on a scene without a texcoord table or without a texture set the
 * pass runs the existing kernels and is the existing entry point bit for bit.
 *  stride       1: the dense pass over `shard` (trx_trace_indirect_rgb_dev's layout and planes); 2..TRX_MAX_AO_STRIDE: the
 *               sparse pass at (stride, phase) over the whole image - shard must be {0, 1, TRX_LAYOUT_IMAGE} - with
 *               trx_trace_indirect_rgb_sparse_dev's low-grid planes.  phase < stride * stride (0 with stride 1).
 *  use_emitters 0: rule 5c, emitter_eps is ignored and n_lights >= 1; 1: rule 5e with emitter_eps, n_lights may be 0 and the
 *               scene needs a current emitter table.  Anything else is refused.
 * It refuses what the corresponding existing entry point refuses. */
int trx_trace_indirect_rgb_textured_dev(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, trx_shard shard,
                                        uint32_t stride, uint32_t phase, uint32_t semantics, uint32_t ray_mask,
                                        const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                        float bounce_eps, float shadow_eps, uint32_t use_emitters, float emitter_eps,
                                        const trx_hit *d_primary, const uint32_t *d_primary_inst, float *d_value_rgb,
                                        void *stream);

/* trx_render_image_colour, _colour_smooth and _colour_emitters in one call, textured (synchronous).  emitter_samples == 0
 * means no emitter sampling (trx_render_image_colour's chain; n_lights >= 1, emitter_eps ignored), otherwise
 * trx_render_image_colour_emitters' chain; smooth (0 / 1) inserts trx_shading_normals_primary_dev after the attribute pass as
 * trx_render_image_colour_smooth does.  Three changes to those chains: trx_surface_albedo_dev runs after the attribute pass
 * (u and v are the same with or without shading normals); the indirect pass is trx_trace_indirect_rgb_textured_dev; the
 * compose is trx_albedo_compose_dev.  The albedo multiplies in the compose, after upsample and filter, so a textured primary
 * albedo stays sharp at any bounce_stride.  On a scene without texcoords or textures the image is the untextured call's byte
 * for byte.  Refusals: those of the chain it stands for, and smooth > 1. */
int trx_render_image_colour_textured(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                                     uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                     uint32_t light_samples, float shadow_eps, float ambient, uint32_t ao_samples, float ao_eps,
                                     float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos,
                                     uint32_t bounce_samples, float bounce_eps, uint32_t bounce_filter_levels,
                                     float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride,
                                     uint32_t bounce_phase, uint32_t bounce_upsample_radius, uint32_t emitter_samples,
                                     float emitter_eps, uint32_t smooth, uint8_t *out_rgba, float *out_ms);

/* Stand-in tables for the generated scenes (host; trx_free'd by the caller).
 * trx_standin_texcoords: box mapping of the mesh as given (verts: n_tris x 9 floats, out_uvs: n_tris x 6).  Per triangle, in
 * binary32 without contraction: e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2) (n.x = e1.y * e2.z - e1.z * e2.y and cyclic); the
 * dominant axis is the one with the largest |n| component, ties going to the lower axis (a NaN component loses to any number; all NaN: x); (s, t) of
 * each corner are its other two coordinates in ascending axis order (axis x: (y, z); y: (x, z); z: (x, y)), bit for bit.  The
 * name is not looked at today.
 * trx_standin_textures: one 64 x 64 TRX_TEX_RGBA8_UNORM, TRX_TEX_BILINEAR checker - texel (x, y) has R = G = B = 255 where
 * ((x >> 3) + (y >> 3)) & 1, otherwise 128, alpha 255 - attached to material 0 only (every other material: TRX_NO_TEXTURE).
 * Refused (TRX_ERR_INVALID): null arguments, n_materials == 0. */
int trx_standin_texcoords(const char *name, const float *verts, uint64_t n_tris, float *out_uvs);
int trx_standin_textures(const char *name, uint32_t n_materials, trx_texture_desc **out_descs, uint32_t *out_n_textures,
                         uint32_t **out_texels, uint64_t *out_n_texels, uint32_t **out_material_texture);

/* trx_load_model with the model's texture coordinates: the same verts and object counts, byte for byte, plus six floats per
 * triangle in that triangle order, (s0, t0, s1, t1, s2, t2) (all trx_free'd by the caller).  OBJ: `vt` records are read (two
 * numbers; a missing second one is +0; nothing is refused - any float is a legal texcoord); the second index of a face corner's
 * v/vt or v/vt/vn names one, relative to the `vt` records read so far when negative.  A corner with no such index (v, v//vn), or
 * with one out of range at that point of the file, gets +0, +0.  A quad's two triangles take corners 0,1,2 and 0,2,3, as for
 * positions.  A JSON model gets +0 everywhere.  *out_has_texcoords is 1 when any corner got a `vt`, else 0.  Refused with
 * TRX_ERR_INVALID: null arguments; TRX_ERR_IO: an unreadable model. */
int trx_load_model_texcoords(const char *path, float **out_verts, uint64_t *out_n_tris, uint64_t **out_object_counts,
                             uint32_t *out_n_objects, float **out_uvs, uint32_t *out_has_texcoords);

/* The `map_Kd` file name of every material of the model, in trx_load_model_materials' material order: *out_names (trx_free'd by
 * the caller) holds *out_n_materials NUL-terminated strings back to back.  An empty string means the material names no map;
 * material 0, the default, never does; a JSON model or an OBJ without readable mtl files gives one empty string.  The name is
 * the last blank-separated word of the `map_Kd` line as it stands in the file (relative to the OBJ's directory by convention):
 * options before it (-s 1 1 1, -clamp on, ...) are skipped, and the last `map_Kd` of a material wins.  The library opens no image
 * file: decoding is the caller's (the command line's --textures).  Refusals as trx_load_model_materials. */
int trx_load_model_material_maps(const char *path, char **out_names, uint32_t *out_n_materials);

/* Status of the most recent trace on this scene (stack overflow is detected
 * in-kernel and latched in device memory).  Synchronises `stream`. */
int trx_scene_check(trx_scene *scene, void *stream);

/* Re-entrancy: the *_dev entry points and trx_traverse1 may be called concurrently on one scene
 * (launch slots); the synchronous entry points below, trx_count_* and trx_bench_primary share
 * per-scene scratch buffers and are serialised by a per-scene lock.
 * Process-wide settings: the builder knobs (trx_set_build_*) live behind one mutex and every build works on
 * the snapshot it took when it started, so setters and builds may run concurrently (a setter only affects
 * builds that start after it returns); trx_flat_build_params never touches them.  trx_set_kernel_variant is a
 * single atomic word read once per launch — a tuning aid: concurrent launches may see either value, results are
 * identical under every value. */

/* ---- tracing: host-buffer convenience (synchronous) --------------------------
 * What rt_gpu_software::start returns to its caller is a time in ms
 * (src/rt_gpu/rt_gpu_software.rs:376); out_ms is the hipEvent time of the
 * kernel(s) (src/timestamp.rs:62-74 equivalent).  out_hits: w*h (or n) host
 * records, may be NULL for timing only. */
int trx_trace_primary(trx_scene *scene, const trx_view *view, uint32_t width,
                      uint32_t height, uint32_t semantics, trx_hit *out_hits,
                      float *out_ms);
int trx_trace_primary_ao(trx_scene *scene, const trx_view *view, uint32_t width,
                         uint32_t height, uint32_t semantics, uint32_t frame, float ao_eps,
                         trx_hit *out_primary, trx_hit *out_ao, float *out_ms);
/* The frame loop of rt_gpu_software::start itself (src/rt_gpu/rt_gpu_software.rs:271-361: per RedrawRequested a
 * primary pass and the AO pass over its hits; --animate advances the noise seed, :285-288), n_frames frames without the
 * host in between.  overlap == 0: both passes of a frame back to back on one stream (what n_frames calls of
 * trx_trace_primary_ao enqueue).  overlap != 0: the AO passes run on a second stream under later frames' primary passes
 * (four primary-hit buffers: the primary passes run up to four frames ahead of the AO passes; same records).  out_primary / out_ao (host, may be NULL): the LAST frame's records;
 * out_ms: hipEvent time from the first launch to the end of the last pass (per frame: / n_frames). */
int trx_frame_loop(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                   uint32_t frame0, int animate, float ao_eps, uint32_t n_frames, int overlap, trx_hit *out_primary,
                   trx_hit *out_ao, float *out_ms);
int trx_trace_rays(trx_scene *scene, const trx_ray *rays, uint64_t n_rays,
                   uint32_t semantics, trx_hit *out_hits, float *out_ms);
/* The same with RayHit.instance_id per hit (u32 arrays, any of them may be NULL; all 0xFFFFFFFF without a TLAS).
 * These are the forms to use on scenes with instance transforms: the AO pass is fed the primary pass's ids. */
int trx_trace_primary_ao_inst(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                              uint32_t semantics, uint32_t frame, float ao_eps, trx_hit *out_primary,
                              uint32_t *out_primary_inst, trx_hit *out_ao, uint32_t *out_ao_inst, float *out_ms);
int trx_trace_rays_inst(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics,
                        trx_hit *out_hits, uint32_t *out_inst, float *out_ms);
/* trx_trace_rays_inst followed by trx_hit_attributes_rays_dev over its hits: out_attr gets one trx_hit_attr per ray
 * (out_hits, out_inst, out_attr may each be NULL); out_ms is the hipEvent time of both passes. */
int trx_trace_rays_attr(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics, trx_hit *out_hits,
                        uint32_t *out_inst, trx_hit_attr *out_attr, float *out_ms);
/* Host-buffer form of trx_trace_occluded_dev. */
int trx_trace_occluded(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics,
                       uint8_t *out_flags, float *out_ms);
/* Host-buffer form of trx_trace_ao_visibility_dev for a whole image: the primary pass and the visibility pass over its
 * records, synchronous (serialised by the per-scene lock like its siblings); out_unoccluded: width * height bytes (may be
 * NULL), out_ms the hipEvent time of both passes. */
int trx_trace_ao_visibility(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                            uint32_t semantics, uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius,
                            uint8_t *out_unoccluded, float *out_ms);
/* Single-ray Traversable::traverse (traversable/src/lib.rs:13-28).  Thread-safe and meant to be called the way the
 * reference calls it - from every worker of a thread pool at once (src/rt_cpu/rt_cpu.rs:35-57).  No call launches
 * anything: the first call starts the scene's RAY SERVICE, a resident kernel that answers out of a ring of 64 slots in
 * pinned host memory (a caller claims a slot, writes its ray, spins on the slot's answer; single- and two-level scenes,
 * one service per semantics word in use) and that a watchdog thread stops 50 ms after the last call - until then a
 * device-wide synchronisation elsewhere in the process (hipDeviceSynchronize, hipFree) waits for it; trx_scene_destroy
 * stops it at once.  A caller blocks for its ray's own walk plus
 * 4 us through host memory, so the rate is (concurrent callers) / (16-45 us): use trx_traverse_batch where the rays can
 * be had together.  primitive_id indexes the PERMUTED triangle
 * list of the hit BLAS (primitive_indices order), exactly like the reference, whose scene structs store their
 * triangles in that order (src/rt_cpu/mod.rs:38-43) and index them with RayHit.primitive_id
 * (src/cwbvh.rs:151-160,177-186); trx_flat.tri_source[blas_tri_start[g] + primitive_id] names the input
 * triangle (with pre-splitting several entries can name the same one). */
int trx_traverse1(trx_scene *scene, const trx_ray *ray, uint32_t semantics,
                  trx_rayhit *out);
/* The same answer for n rays in ONE launch: what rt_cpu::start's pixel loop (src/rt_cpu/rt_cpu.rs:35-92) should call
 * instead of n device round trips - generate the frame's rays, traverse them here, shade from the RayHits (which
 * carry geometry_id / instance_id exactly like trx_traverse1's).  Host buffers; out_ms (may be NULL) is the hipEvent
 * time of the traversal. */
int trx_traverse_batch(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t semantics,
                       trx_rayhit *out, float *out_ms);

/* Benchmark loop of the reference (warm-up dispatch + timestamp pair per
 * frame, min and mean over frames: src/rt_gpu/rt_gpu_software.rs:289-302,
 * 339-344,376).  Traces `frames` primary frames after `warmup` untimed ones
 * into an internal device buffer; returns min / mean kernel ms. */
int trx_bench_primary(trx_scene *scene, const trx_view *view, uint32_t width,
                      uint32_t height, uint32_t semantics, uint32_t warmup,
                      uint32_t frames, float *out_min_ms, float *out_mean_ms);

/* Development entry points (per-wave timelines, footprints, tile profiles, the kernel-variant tuning word) are NOT part
 * of the boundary a tray_racing host binds: they live in include/trx_dev.h. */

/* ---- multi-GPU: the hit-shard gather -----------------------------------------
 * tray_racing is single-GPU; these entry points are the north_star's "RCCL only for the final hit-buffer gather"
 * in a form a Rust / C host can drive: one process per GPU, rank r traces
 * trx_shard{r, N, TRX_LAYOUT_SHARD} of every frame of a batch straight into its block of a gather buffer laid out
 * [N][m][R] (R = trx_shard_tiles(w, h, {0, N}) * 64 records, the same on every rank), ONE in-place all-gather per
 * batch completes the m frames on every rank, and trx_assemble_frames de-interleaves them into row-major frames.
 * RCCL (librccl.so) is loaded on first use; a single-GPU host never touches it.  The environment variable
 * TRX_RCCL_LIBRARY, when set, names the library to load instead of the system's librccl.so; a library that cannot be
 * loaded makes every trx_comm_* call return TRX_ERR_NO_DEVICE with the loader's message. */
typedef struct trx_comm trx_comm;
/* 128 opaque bytes (ncclUniqueId): produced on rank 0, handed to the other ranks by the host's own means. */
int trx_comm_unique_id(void *out_id128);
/* Collective over all ranks (ncclCommInitRank).  device: the HIP device of this rank. */
int trx_comm_create(const void *id128, int rank, int world, int device, trx_comm **out);
void trx_comm_destroy(trx_comm *comm);
int trx_comm_world_size(const trx_comm *comm); /* as the communicator reports it */
/* In-place all-gather (ncclAllGather over xGMI) of `records_per_rank` hit records per rank, enqueued on `stream`:
 * d_flat holds world blocks of records_per_rank records, this rank's block (already written by its trace launches)
 * at rank * records_per_rank.  For a batch of m frames records_per_rank = m * R. */
int trx_gather_shards(trx_comm *comm, trx_hit *d_flat, uint64_t records_per_rank, void *stream);
/* The same gather to ONE rank (SURVEY 8(e)'s alternative: ncclSend / ncclRecv in one group): rank `root` receives the
 * other ranks' blocks into d_flat, every other rank sends its own block and receives nothing, so a host that
 * consumes the frames on one GPU moves 1/world of the all-gather's bytes.  Only the root may then assemble. */
int trx_gather_shards_root(trx_comm *comm, trx_hit *d_flat, uint64_t records_per_rank, int root, void *stream);
/* De-interleave a gathered [world][n_frames][records_per_frame] buffer into n_frames row-major width x height
 * frames (d_frames: n_frames * width * height records), enqueued on `stream`.  Needs no communicator: with
 * world == 1 it turns one shard-layout frame into an image-layout one. */
int trx_assemble_frames(const trx_hit *d_flat, uint64_t records_per_frame, uint32_t width, uint32_t height,
                        uint32_t world, uint32_t n_frames, trx_hit *d_frames, void *stream);

/* ---- host side: CWBVH construction (CPU) -------------------------------------
 * Stands in for obvhs build_cwbvh_from_tris / build_cwbvh (called at
 * src/cwbvh.rs:97,132), which the Rust host keeps doing in a real
 * integration.  Node encoding follows embree/src/bvh_embree_to_cwbvh.rs:85-186
 * and child ordering embree/src/bvh_embree.rs:284-349. */
typedef struct trx_bvh trx_bvh; /* opaque CwBvh {nodes, primitive_indices, total_aabb} */

/* verts: n_tris * 9 floats (v0,v1,v2).  max_prims_per_leaf 1..3
 * (src/main.rs:176-178).  threads <= 0: all cores. */
int trx_bvh_build_tris(const float *verts, uint64_t n_tris, uint32_t max_prims_per_leaf,
                       int threads, trx_bvh **out);
/* aabbs: n * 6 floats (min xyz, max xyz) — the TLAS build over BLAS AABBs
 * (src/cwbvh.rs:114,132). */
int trx_bvh_build_aabbs(const float *aabbs, uint64_t n, uint32_t max_prims_per_leaf,
                        int threads, trx_bvh **out);
/* SAH weights of the 8-wide collapse for subsequent builds (process-wide): cost of visiting a node
 * and of testing one primitive, the knobs behind the reference's --collapse-traversal-cost
 * (src/main.rs:158-163, swept by src/auto_tune.rs:20-28).  Defaults 1.0 / 0.3. */
int trx_set_build_costs(float traversal_cost, float prim_cost);
/* BVH2 reinsertion pass for subsequent builds (process-wide): per iteration the `batch_ratio`
 * fraction of the nodes with the largest area is re-placed where the tree's summed area drops the
 * most (Meister & Bittner 2018) — obvhs' `reinsertion_batch_ratio`, the reference's `-r`
 * (src/main.rs:113-118).  batch_ratio 0 switches the pass off.  Default 0.02 x 4 iterations.  Applied to
 * triangle builds only: over instance boxes (TLAS) it measured worse and is skipped. */
int trx_set_build_reinsertion(float batch_ratio, int iterations);
/* How the candidates of a reinsertion iteration are batched, for subsequent builds (process-wide).  0 (default): the
 * pipeline's own way - one at a time, each search on the tree the previous move left (trx_flat_build and the presets), or
 * batches of 128 searched concurrently (trx_flat_build_params).  1: ONE batch per iteration - every candidate searches
 * the tree the previous iteration left, the paper's formulation - and the searches run as a kernel on the build device
 * when one is set (trx_set_build_device; one thread per candidate), on the host cores otherwise: the same tree either
 * way.  An iteration gains less than with small batches (more searches are stale when their moves are applied), so give
 * the pass more of them (trx_set_build_reinsertion). */
int trx_set_build_reinsertion_batches(int whole_iterations);
/* The reference's --preset names (src/main.rs:125-131,563-570: "fastest_build" ... "very_slow_build", "" =
 * defaults) mapped onto this builder's knobs — SAH bins, exact-sweep threshold, reinsertion ratio and
 * iterations, pre-splitting (on from "slow_build"); "medium_build" is the default setting and "" restores it.
 * Process-wide, for subsequent builds. */
int trx_set_build_preset(const char *name);
/* Pre-splitting (obvhs `pre_split`, the reference's --split, src/main.rs:572): triangles whose boxes are mostly
 * empty are cut into several references with clipped, tighter boxes before the build, at most `extra_ratio` x
 * n_tris extra references (0 = off, the reference's default).  Such triangles then appear more than once in
 * the permuted triangle buffer of trx_flat (`tri_source` still names the input triangle).  Triangle builds
 * only; process-wide, for subsequent builds. */
int trx_set_build_split(float extra_ratio);
void trx_bvh_destroy(trx_bvh *bvh);
uint64_t trx_bvh_node_count(const trx_bvh *bvh);
uint64_t trx_bvh_prim_count(const trx_bvh *bvh);
const void *trx_bvh_nodes(const trx_bvh *bvh);                 /* node_count * 80 B */
const uint32_t *trx_bvh_primitive_indices(const trx_bvh *bvh); /* prim_count u32     */
void trx_bvh_total_aabb(const trx_bvh *bvh, float out6[6]);
double trx_bvh_build_seconds(const trx_bvh *bvh);

/* cwbvh_gpu_runner (src/rt_gpu/mod.rs:16-112) as one call: builds one BLAS per
 * object (or one flattened BLAS when use_tlas == 0, src/main.rs:300-308),
 * permutes triangles into primitive_indices order, offsets primitive_base_idx,
 * optionally builds the TLAS and concatenates, and returns the flat buffers
 * the GPU path consumes.  Output arrays are owned by the trx_flat and freed
 * with trx_flat_destroy. */
typedef struct trx_flat {
    void *bvh_bytes;
    uint64_t n_nodes;
    float *tri_verts;        /* n_tris * 9 floats, TRX_TRI_VERTS_36, permuted */
    uint64_t n_tris;
    uint32_t *instance_offsets;
    uint32_t n_instances;
    uint32_t tlas_start;
    uint32_t *tri_source;    /* n_tris: index of each permuted triangle in the input */
    uint32_t *blas_tri_start;/* n_blas + 1: first permuted triangle of each BLAS (geometry_id lookup) */
    uint32_t n_blas;
    double blas_build_s;
    double tlas_build_s;
    float *tri_boxes;        /* n_tris * 6 floats (min xyz, max xyz): the box each triangle entry was built with —
                              * its own, or the clipped part a pre-split reference covers (trx_set_build_split) */
    uint32_t *instance_source;   /* n_instances: which of the caller's objects (trx_flat_build) or instances
                                  * (trx_flat_build_instanced) TLAS primitive k is */
    float *instance_transforms;  /* n_instances * 16 (object-to-world, column-major) in TLAS-primitive order, ready for
                                  * trx_scene_set_instance_transforms; NULL when no transforms were given */
    uint32_t *instance_entry_nodes; /* n_instances, ready for trx_scene_set_instance_entry_nodes: the node of its BLAS at
                                     * which TLAS primitive k starts (re-braided TLAS, trx_set_build_rebraid); NULL when
                                     * every primitive is a whole BLAS (the reference's layout) */
} trx_flat;
/* Every flat builder below (trx_flat_build, trx_flat_build_instanced, trx_flat_build_params,
 * trx_flat_build_preset_device), like trx_bvh_build_tris, refuses a non-finite vertex coordinate (NaN, +-inf) with TRX_ERR_INVALID, as
 * trx_scene_refit does: nothing is built and *out is left as it was.  Finite degenerate geometry - duplicates, points,
 * segments, boxes without extent, coordinates whose box areas underflow to 0 or overflow to +inf, signed zeros - is
 * built.  A collapsed tree deeper than 512 levels (the depth the validators and the traversal stacks are sized for) is
 * refused with TRX_ERR_INVALID as well, not returned. */
int trx_flat_build(const float *verts, const uint64_t *object_tri_counts, uint32_t n_objects,
                   int use_tlas, uint32_t max_prims_per_leaf, int threads, trx_flat **out);
void trx_flat_destroy(trx_flat *flat);
/* One BLAS per object and a TLAS over n_instances INSTANCES of them (true instancing: several instances may name
 * the same object).  instance_object[k] = object of instance k; instance_object_to_world = n_instances column-major
 * affine 4x4 matrices (NULL = all identity).  TLAS boxes bound the transformed BLAS boxes.  The result's
 * instance_offsets / instance_transforms / instance_source are in TLAS-primitive order. */
int trx_flat_build_instanced(const float *verts, const uint64_t *object_tri_counts, uint32_t n_objects,
                             const uint32_t *instance_object, const float *instance_object_to_world,
                             uint32_t n_instances, uint32_t max_prims_per_leaf, int threads, trx_flat **out);

/* The reference's BvhBuildParams (src/main.rs:571-585), field for field, for callers that carry one around.
 * trx_flat_build_params runs the ploc_cwbvh pipeline with them: Morton sort at sort_precision bits (64 | 128,
 * "Unsupported sort precision" otherwise, src/main.rs:576-580), PLOC merging with ploc_search_distance (1..32)
 * places either side and distance 1 for the first search_depth_threshold rounds, reinsertion at
 * reinsertion_batch_ratio, optional pre_split, collapse to <= max_prims_per_leaf triangles per leaf at
 * collapse_traversal_cost.  post_collapse_reinsertion_batch_ratio_multiplier is "For BVH2 only" in the reference
 * (src/main.rs:119-123) and has no effect on a CWBVH build. */
typedef struct trx_build_params {
    uint32_t pre_split;                 /* --split */
    uint32_t ploc_search_distance;      /* --search-distance */
    uint32_t search_depth_threshold;    /* --search-depth-threshold */
    float reinsertion_batch_ratio;      /* -r */
    uint32_t sort_precision;            /* --sort-precision: 64 | 128 */
    uint32_t max_prims_per_leaf;        /* --max-prims-per-leaf: 1..3 for CWBVH */
    float post_collapse_reinsertion_batch_ratio_multiplier;
    float collapse_traversal_cost;      /* --collapse-traversal-cost */
} trx_build_params;
void trx_build_params_default(trx_build_params *params); /* the reference's command-line defaults */
/* Which stages of subsequent builds run on a HIP device, as kernels (process-wide): device >= 0 = that device, -1 = the
 * host cores only (default).  Objects of at least 32,768 primitives take the device stages; the many small BLASes of a
 * TLAS scene stay on the host cores.  Stages: the BVH2 stage of trx_flat_build_params (Morton sort + PLOC merge rounds);
 * the whole-iteration reinsertion pass (trx_set_build_reinsertion_batches(1)) with the tree resident on the device -
 * candidate selection, searches, the choice and application of the moves, the boxes; and, for every builder, the BVH2 -> CWBVH stage (cost table,
 * collapse, slot assignment, node encoding, primitive order).  Each device stage returns the very bytes its host twin
 * returns (same operations in the same order), so a build is the same build wherever it ran.  A device failure fails
 * the build (TRX_ERR_NO_DEVICE / TRX_ERR_OOM): nothing falls back silently. */
int trx_set_build_device(int device);
/* TLAS of trx_flat_build / trx_flat_build_params (process-wide): a BLAS whose box exceeds `area_fraction` of the scene
 * box's surface area is referenced through the subtrees under its root instead of as a whole, largest first, as long as
 * the opened node has inner children only; trx_flat.instance_entry_nodes then names each primitive's entry node.
 * Default 1/4096; 0 = never (every primitive a whole BLAS, as the reference builds it, src/cwbvh.rs:108-137).  Instanced
 * builds (trx_flat_build_instanced) are never re-braided. */
int trx_set_build_rebraid(float area_fraction);
int trx_flat_build_params(const float *verts, const uint64_t *object_tri_counts, uint32_t n_objects,
                          int use_tlas, const trx_build_params *params, int threads, trx_flat **out);

/* A preset's build with every stage on HIP device `device` (the ploc_cwbvh pipeline: Morton sort + PLOC rounds with the
 * reference's search parameters, src/main.rs:85-98; reinsertion in whole-iteration batches; collapse + encoding) and a
 * reinsertion budget per preset name (src/main.rs:565-570): bistro-class medium_build in 0.4 s against 0.96 s on 16 host
 * cores, walked with no more node visits.  device < 0: the same pipeline on the host cores (same bytes). */
int trx_flat_build_preset_device(const float *verts, const uint64_t *object_tri_counts, uint32_t n_objects, int use_tlas,
                                 const char *preset, uint32_t max_prims_per_leaf, int threads, int device, trx_flat **out);

/* ---- host side: scenes ----------------------------------------------------
 * The reference's assets are absent: seeded procedural
 * stand-ins with the triangle counts of README.md:27-34.  name is one of
 * "cornell" "demoscene" "kitchen" "bistro" "hairball" "san_miguel" "soup".
 * Returns a malloc'd vertex array (n_tris*9 floats) and per-object triangle
 * counts; free with trx_free. */
int trx_gen_scene(const char *name, uint64_t n_tris_target, uint64_t seed, float **out_verts,
                  uint64_t *out_n_tris, uint64_t **out_object_counts, uint32_t *out_n_objects);
/* Camera of assets/scenes/<name>.ron (eye, look_at, fov) for the stand-in. */
int trx_scene_camera(const char *name, float eye[3], float look_at[3], float *fov_deg);
/* load_meshs (src/main.rs:494-561): Wavefront OBJ (tri + quad fan, one object
 * per `o`) or the JSON triangle list. */
int trx_load_model(const char *path, float **out_verts, uint64_t *out_n_tris,
                   uint64_t **out_object_counts, uint32_t *out_n_objects);
/* A scene file of the reference (assets/scenes/<name>.ron: model_path, camera) as src/main.rs:259-298 reads it: the
 * camera, and the model loaded from the path the reference's rule gives (scene path and model path both relative: the
 * model is taken relative to the scene file's great-grandparent directory, src/main.rs:271-284). */
int trx_load_scene(const char *path, float **out_verts, uint64_t *out_n_tris, uint64_t **out_object_counts,
                   uint32_t *out_n_objects, float eye[3], float look_at[3], float *fov_deg);
void trx_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* TRX_H */
