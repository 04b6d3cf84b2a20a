// api.cpp - the C-ABI declared in include/trx.h: errors, devices, scene upload (replaces the buffer creation of
// src/rt_gpu/rt_gpu_software.rs:83-160) and its setters, the camera (src/main.rs:602-616).  The other entry points
// live in api_launch.cpp / api_trace.cpp / api_traverse.cpp / api_build.cpp (api_internal.h says which is where).
// There is deliberately no CPU traversal in this library.
#include "api_internal.h"

namespace {
thread_local std::string g_err;
} // namespace

namespace trxapi {
std::atomic<uint32_t> g_variant{0};
std::string &err_string() { return g_err; }
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
} // namespace trxapi

namespace trx {
// error reporting for the other translation units of the library (comm.cpp)
int fail_msg(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
} // namespace trx

namespace trxapi {

// Structural validation of untrusted node buffers: a kernel that walks a
// malformed tree would read out of bounds (and can take the GPU down), so
// every index the kernel can form is range-checked here once.
int validate_nodes(const CwbvhNode *nodes, uint64_t n_nodes, uint64_t n_tris, const uint32_t *inst,
                   uint32_t n_inst, uint32_t tlas_start) {
    std::vector<uint32_t> seg; // BLAS segment starts, sorted
    const bool tlas = n_inst > 0;
    if (tlas) {
        if (tlas_start >= n_nodes) return fail(TRX_ERR_FORMAT, "tlas_start %u >= n_nodes %llu", tlas_start, (unsigned long long)n_nodes);
        seg.assign(inst, inst + n_inst);
        for (uint32_t o : seg)
            if (o >= tlas_start) return fail(TRX_ERR_FORMAT, "instance offset %u not below tlas_start %u", o, tlas_start);
        std::sort(seg.begin(), seg.end());
        seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
    }
    for (uint64_t i = 0; i < n_nodes; i++) {
        const CwbvhNode &n = nodes[i];
        uint64_t seg_begin = 0, seg_end = n_nodes;
        bool in_tlas = false;
        if (tlas) {
            if (i >= tlas_start) {
                seg_begin = tlas_start;
                in_tlas = true;
            } else {
                auto it = std::upper_bound(seg.begin(), seg.end(), (uint32_t)i);
                seg_begin = it == seg.begin() ? 0 : *(it - 1);
                seg_end = it == seg.end() ? tlas_start : *it;
            }
        }
        uint32_t inner = 0, prims = 0;
        for (int s = 0; s < 8; s++) {
            uint8_t m = n.child_meta[s];
            if (m == 0) continue;
            if ((m & 0x18) == 0x18) {
                inner++;
            } else {
                uint32_t bits = m >> 5, cnt = bits == 1 ? 1 : bits == 3 ? 2 : bits == 7 ? 3 : 0;
                if (!cnt) return fail(TRX_ERR_FORMAT, "node %llu slot %d: bad leaf meta 0x%02x", (unsigned long long)i, s, m);
                prims = std::max(prims, (uint32_t)(m & 0x1f) + cnt);
            }
        }
        if (inner != (uint32_t)__builtin_popcount(n.imask))
            return fail(TRX_ERR_FORMAT, "node %llu: imask 0x%02x disagrees with child_meta", (unsigned long long)i, n.imask);
        if (inner && (uint64_t)n.child_base_idx + inner > seg_end - seg_begin)
            return fail(TRX_ERR_FORMAT, "node %llu: children [%u,+%u) leave the BVH segment", (unsigned long long)i, n.child_base_idx, inner);
        if (prims > 24) return fail(TRX_ERR_FORMAT, "node %llu: more than 24 primitives", (unsigned long long)i);
        uint64_t limit = in_tlas ? n_inst : n_tris;
        if (prims && (uint64_t)n.primitive_base_idx + prims > limit)
            return fail(TRX_ERR_FORMAT, "node %llu: primitives [%u,+%u) out of range %llu", (unsigned long long)i,
                        n.primitive_base_idx, prims, (unsigned long long)limit);
    }
    return TRX_OK;
}

} // namespace trxapi

namespace {

float half_to_float(uint16_t h) {
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1f, man = h & 0x3ffu, bits;
    if (exp == 0) {
        if (man == 0) {
            bits = sign;
        } else {
            float f = (float)man * 5.9604644775390625e-8f;
            return sign ? -f : f;
        }
    } else if (exp == 31) {
        bits = sign | 0x7f800000u | (man << 13);
    } else {
        bits = sign | ((exp + 112) << 23) | (man << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

// Any accepted input format -> 48-byte device record {v0, e1 = v0 - v1, e2 = v2 - v0, ng = e1 x e2 in the w lanes}.
void convert_tris(const void *src, uint64_t n, uint32_t fmt, TriDev *dst) {
    const uint8_t *b = (const uint8_t *)src;
    for (uint64_t i = 0; i < n; i++) {
        TriDev t;
        std::memset(&t, 0, sizeof(t));
        if (fmt == TRX_TRI_F16_24) {
            float v[3];
            uint32_t e[3];
            std::memcpy(v, b + 24 * i, 12);
            std::memcpy(e, b + 24 * i + 12, 12);
            for (int k = 0; k < 3; k++) {
                t.v0[k] = v[k];
                t.e1[k] = -half_to_float((uint16_t)(e[k] >> 16)); // stored e1 = v1 - v0
                t.e2[k] = half_to_float((uint16_t)(e[k] & 0xffff));
            }
        } else {
            float v[9];
            std::memcpy(v, b + 36 * i, 36);
            for (int k = 0; k < 3; k++) {
                t.v0[k] = v[k];
                if (fmt == TRX_TRI_VERTS_36) {
                    t.e1[k] = v[k] - v[3 + k];
                    t.e2[k] = v[6 + k] - v[k];
                } else {
                    t.e1[k] = v[3 + k];
                    t.e2[k] = v[6 + k];
                }
            }
        }
        t.ngx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
        t.ngy = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
        t.ngz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
        dst[i] = t;
    }
}

} // namespace

extern "C" {

const char *trx_last_error(void) { return g_err.c_str(); }
uint32_t trx_abi_version(void) { return TRX_ABI_VERSION; }

int trx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int trx_device_name(int device, char *buf, size_t buf_len) {
    if (!buf || !buf_len) return fail(TRX_ERR_INVALID, "null buffer");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buf_len, "%s", prop.gcnArchName);
    return TRX_OK;
}

uint32_t trx_tri_format_bytes(uint32_t f) {
    switch (f) {
    case TRX_TRI_F16_24: return 24;
    case TRX_TRI_VERTS_36: return 36;
    case TRX_TRI_EDGES_36: return 36;
    default: return 0;
    }
}

uint32_t trx_shard_tiles(uint32_t w, uint32_t h, trx_shard shard) {
    if (shard.count == 0) shard.count = 1;
    const uint64_t tiles = (uint64_t)((w + 7) / 8) * ((h + 7) / 8);
    if (shard.index >= shard.count || tiles <= shard.index) return 0;
    return (uint32_t)((tiles - shard.index + shard.count - 1) / shard.count);
}

uint32_t trx_set_kernel_variant(uint32_t variant) {
    return g_variant.exchange(variant);
}

int trx_scene_create(const void *bvh_bytes, uint64_t n_nodes, const void *tri_bytes, uint64_t n_tris,
                     uint32_t tri_format, const uint32_t *instance_offsets, uint32_t n_instances,
                     uint32_t tlas_start, int device, trx_scene **out) {
    if (!out) return fail(TRX_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!bvh_bytes || n_nodes == 0) return fail(TRX_ERR_INVALID, "empty node buffer");
    if (n_tris && !tri_bytes) return fail(TRX_ERR_INVALID, "tri_bytes is null");
    if (!trx_tri_format_bytes(tri_format)) return fail(TRX_ERR_INVALID, "unknown tri_format %u", tri_format);
    if (n_nodes >= 0xffffffffull || n_tris >= 0xffffffffull) return fail(TRX_ERR_INVALID, "buffer too large for u32 indices");
    if (n_instances && !instance_offsets) return fail(TRX_ERR_INVALID, "instance_offsets is null");
    if (!n_instances && tlas_start != 0) return fail(TRX_ERR_INVALID, "tlas_start without instances");
    int rc = validate_nodes((const CwbvhNode *)bvh_bytes, n_nodes, n_tris, instance_offsets, n_instances, tlas_start);
    if (rc) return rc;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(TRX_ERR_NO_DEVICE, "no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(TRX_ERR_INVALID, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));

    // (a failure below destroys the half-made scene: its members release what was created)
    std::unique_ptr<trx_scene, void (*)(trx_scene *)> s(new (std::nothrow) trx_scene(), trx_scene_destroy);
    if (!s) return fail(TRX_ERR_OOM, "host allocation failed");
    s->device = device;
    s->n_nodes = n_nodes;
    s->n_tris = n_tris;
    s->n_inst = n_instances;
    s->tlas_start = tlas_start;
    s->tlas = n_instances > 0;
    s->tri_format = tri_format;

    std::vector<TriDev> tris(std::max<uint64_t>(n_tris, 1));
    convert_tris(tri_bytes, n_tris, tri_format, tris.data());

    static_assert(TRX_NODE_BYTES % sizeof(uint4) == 0 && sizeof(TriDev) % sizeof(float4) == 0, "records of whole vectors");
    HIP_TRY(s->nodes.alloc(n_nodes * (TRX_NODE_BYTES / sizeof(uint4))));
    HIP_TRY(hipMemcpy(s->nodes.get(), bvh_bytes, n_nodes * TRX_NODE_BYTES, hipMemcpyHostToDevice));
    HIP_TRY(s->tris.alloc(tris.size() * (sizeof(TriDev) / sizeof(float4))));
    HIP_TRY(hipMemcpy(s->tris.get(), tris.data(), tris.size() * sizeof(TriDev), hipMemcpyHostToDevice));
    uint32_t zero = 0;
    if (n_instances) s->h_inst.assign(instance_offsets, instance_offsets + n_instances);
    HIP_TRY(s->inst.alloc(std::max<uint32_t>(n_instances, 4)));
    HIP_TRY(hipMemcpy(s->inst.get(), n_instances ? instance_offsets : &zero, (n_instances ? n_instances : 1) * sizeof(uint32_t),
                      hipMemcpyHostToDevice));
    HIP_TRY(s->ev0.create());
    HIP_TRY(s->ev1.create());
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
        s->cu_count = prop.multiProcessorCount;
    }
    s->grid = trace_grid_size(device, 0, s->tlas, 0, false);
    {   // extent of the root node's quantisation frame (255 steps of 2^(e - 127) per axis): the scene's scale
        const CwbvhNode &root = ((const CwbvhNode *)bvh_bytes)[s->tlas ? tlas_start : 0];
        double d2 = 0.0;
        for (int k = 0; k < 3; k++) {
            const double ext = 255.0 * std::ldexp(1.0, (int)root.e[k] - 127);
            d2 += ext * ext;
        }
        s->scene_diag = (float)std::sqrt(d2);
    }
    {   // may the literal-division node test multiply e = 2^(byte - 127) by the ray's 1/d instead of dividing by d?  Exact
        // while the product stays normal: exponent bytes 0 (e = 0) or >= 21 with |1/d| >= 2^-20 (kernels.hip, pow2)
        bool ok = true;
        const CwbvhNode *nodes = (const CwbvhNode *)bvh_bytes;
        for (uint64_t i = 0; i < n_nodes && ok; i++)
            for (int k = 0; k < 3; k++) ok = ok && (nodes[i].e[k] == 0 || nodes[i].e[k] >= 21);
        // ... and may it compute (p - o) / d from the ray's 1/d by one correction step (kernels.hip, div_by_rcp)?  Every
        // component of every node's p is +0 or 2^-36 <= |p| <= 2^59 (no -0, no NaN, nothing tiny or enormous): with the
        // ray's own flag (origin components 0 or in the same range) p - o is then +0 or 2^-59 <= |p - o| <= 2^60
        bool org = ok;
        for (uint64_t i = 0; i < n_nodes && org; i++)
            for (int k = 0; k < 3; k++) {
                uint32_t bits;
                std::memcpy(&bits, &nodes[i].p[k], 4);
                const float a = std::fabs(nodes[i].p[k]);
                org = org && (bits == 0u || (a >= 0x1p-36f && a <= 0x1p59f));
            }
        s->exp_exact = ok ? (org ? 2u : 1u) : 0u;
    }
    if (s->grid <= 0) return fail(TRX_ERR_NO_DEVICE, "could not size the persistent grid");
    *out = s.release();
    return TRX_OK;
}

void trx_scene_destroy(trx_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (RayService *&v : s->svc) { // (resident kernels first: the device-wide synchronisation below would wait for them)
        delete v;
        v = nullptr;
    }
    (void)hipDeviceSynchronize();
    delete s; // (every buffer, event and stream of the scene goes with its members, after the synchronisation above)
}

uint64_t trx_scene_device_bytes(const trx_scene *s) {
    if (!s) return 0;
    uint64_t bytes = s->n_nodes * TRX_NODE_BYTES + s->n_tris * sizeof(TriDev) + (uint64_t)s->n_inst * 4;
    // launch slots claimed so far: stack spill areas and tile-order lists
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    bytes += s->inst_mask.count(); // the instance mask table (trx_scene_set_instance_masks; swapped under mu)
    // the material table and the triangles' indices (trx_scene_set_materials; swapped under mu)
    bytes += s->materials.count() * sizeof(trx_material) + s->tri_material.count() * sizeof(uint16_t);
    bytes += s->emitters.count() * sizeof(float4) + s->emitter_cdf.count() * sizeof(float); // the emitter table (trx_scene_build_emitters; swapped under mu)
    bytes += s->vertex_normals.count() * sizeof(float4); // the vertex normals, 48 B per triangle (trx_scene_set_vertex_normals; swapped under mu)
    bytes += s->texcoords.count() * sizeof(float2); // the texture coordinates, 24 B per triangle (trx_scene_set_texcoords; swapped under mu)
    // the texture set (trx_scene_set_textures; swapped under mu): descriptors, texels, the per-material index, the sRGB table
    bytes += s->tex_descs.count() * sizeof(uint4) + (s->texels.count() + s->material_texture.count()) * sizeof(uint32_t) +
             s->tex_srgb.count() * sizeof(float);
    bytes += s->image_thr.count() * sizeof(float); // the shade's code thresholds (api_image.cpp)
    for (const Slot &sl : s->slots) {
        bytes += sl.spill.count() * sizeof(uint2) + sl.ctr.count() * sizeof(SlotCounters);
        bytes += sl.ao_rays.count() * sizeof(trx_ray) + sl.ao_flags.count(); // the AO visibility pass's scratch (api_ao.cpp)
        // the indirect pass's scratch (api_ao.cpp)
        bytes += sl.gi_rays.count() * sizeof(trx_ray) + sl.gi_hits.count() * sizeof(trx_hit) + sl.gi_inst.count() * sizeof(uint32_t) +
                 sl.gi_attr.count() * sizeof(trx_hit_attr) + (sl.gi_sum.count() + sl.gi_acc.count()) * sizeof(float);
        bytes += (sl.em_wgeo.count() + sl.em_acc.count()) * sizeof(float) + sl.em_pick.count() * sizeof(uint32_t); // the emitter passes' scratch
        bytes += sl.vf_plane.count() * sizeof(float); // the value filter's plane of an aliased base (api_image.cpp)
        for (const auto &o : sl.order) bytes += o.lists.count() * sizeof(uint32_t);
    }
    // trx_frame_loop's record buffers (four primary, one AO; instance ids beside them on two-level scenes)
    bytes += s->loop.records * (FrameLoop::kBuffers + 1) * (sizeof(trx_hit) + (s->tlas ? sizeof(uint32_t) : 0));
    // trx_scene_refit's schedule and node boxes (after the first refit)
    bytes += refit_state_bytes(s);
    return bytes;
}
int trx_scene_device(const trx_scene *s) { return s ? s->device : -1; }

int trx_scene_set_geometry_ranges(trx_scene *s, const uint32_t *blas_tri_start, uint32_t n_blas) {
    if (!s || (!blas_tri_start && n_blas)) return fail(TRX_ERR_INVALID, "null argument");
    s->blas_tri_start.assign(blas_tri_start, blas_tri_start + n_blas + (n_blas ? 1 : 0));
    return TRX_OK;
}

} // extern "C"

// The scene under a launch slot's frozen tile order changed (instances moved, entry nodes replaced): the next frame of
// every slot files a new order even if its camera has not moved - an order learnt for other geometry is only stale, never
// wrong, but a static camera would replay it for ever.  Call with s->mu held.
void trxapi::forget_tile_orders(trx_scene *s) {
    for (Slot &sl : s->slots)
        for (auto &o : sl.order) o.have_views = false;
}

// A device table swapped out under s->mu is freed once `waited` (the wait for the kernels that may read it) succeeded;
// after a failed wait it is kept rather than freed under a kernel that may still read it.
template <typename T>
static hipError_t retire(DevBuf<T> &old, hipError_t waited) {
    if (waited == hipSuccess) old.reset();
    else (void)old.release();
    return waited;
}

// A scene's texture set (trx_scene_set_textures) on its way in or out: the four device tables, which are swapped and retired
// together.  Call take_from / give_to with s->mu held.
struct TextureSet {
    DevBuf<uint4> descs;
    DevBuf<uint32_t> texels, material_texture;
    DevBuf<float> srgb;
    std::vector<trx_texture_desc> h_descs;
    std::vector<uint32_t> h_texels, h_material_texture;
    void take_from(trx_scene *s) { // (no-throw: moves and swaps only; the scene is left without a set)
        descs = std::move(s->tex_descs), texels = std::move(s->texels);
        material_texture = std::move(s->material_texture), srgb = std::move(s->tex_srgb);
        h_descs.swap(s->h_tex_descs), h_texels.swap(s->h_texels), h_material_texture.swap(s->h_material_texture);
        s->h_tex_descs.clear(), s->h_texels.clear(), s->h_material_texture.clear();
    }
    void give_to(trx_scene *s) {
        s->tex_descs = std::move(descs), s->texels = std::move(texels);
        s->material_texture = std::move(material_texture), s->tex_srgb = std::move(srgb);
        s->h_tex_descs.swap(h_descs), s->h_texels.swap(h_texels), s->h_material_texture.swap(h_material_texture);
    }
    hipError_t retire_all(hipError_t waited) {
        (void)retire(descs, waited), (void)retire(texels, waited), (void)retire(material_texture, waited);
        return retire(srgb, waited);
    }
};

extern "C" {

// Entry nodes: TLAS primitive k starts its BLAS walk at node entry_nodes[k] of the BLAS at instance_offsets[k] instead
// of node 0, so one BLAS can be referenced as several subtrees (re-braiding: a BLAS whose box spans the scene no longer
// makes every ray enter it at the root).  Validated like the node buffer: an entry must lie inside its BLAS segment.
int trx_scene_set_instance_entry_nodes(trx_scene *s, const uint32_t *entry_nodes, uint32_t n) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    DevBuf<uint32_t> fresh;
    std::vector<uint32_t> host_copy;
    if (entry_nodes && n) {
        if (!s->tlas) return fail(TRX_ERR_INVALID, "entry nodes need a TLAS scene");
        if (n != s->n_inst) return fail(TRX_ERR_INVALID, "%u entry nodes for %u instances", n, s->n_inst);
        std::vector<uint32_t> seg(s->h_inst);
        std::sort(seg.begin(), seg.end());
        seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
        for (uint32_t k = 0; k < n; k++) {
            auto it = std::upper_bound(seg.begin(), seg.end(), s->h_inst[k]);
            const uint32_t seg_end = it == seg.end() ? s->tlas_start : *it;
            if ((uint64_t)s->h_inst[k] + entry_nodes[k] >= seg_end)
                return fail(TRX_ERR_FORMAT, "instance %u: entry node %u leaves its BLAS [%u, %u)", k, entry_nodes[k], s->h_inst[k], seg_end);
        }
        try { // (host copy for the refit's schedule, which follows the walk into the entry nodes; taken before the swap)
            host_copy.assign(entry_nodes, entry_nodes + n);
        } catch (const std::exception &) {
            return fail(TRX_ERR_OOM, "host allocation failed");
        }
        HIP_TRY(fresh.alloc(n));
        const hipError_t e = hipMemcpy(fresh.get(), entry_nodes, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the entry nodes failed: %s", hipGetErrorString(e));
    }
    DevBuf<uint32_t> old;
    {   // swapped under the launch mutex, freed after every kernel enqueued before the swap has drained
        std::lock_guard<std::mutex> lock(s->mu);
        old = std::move(s->inst_entry);
        s->inst_entry = std::move(fresh);
        s->h_inst_entry.swap(host_copy); // (no-throw: device and host copies change together)
        s->inst_entry_version++;
        s->emitters_stale = true; // (an instance's triangles are those reachable from its entry node)
        forget_tile_orders(s);
    }
    HIP_TRY(retire(old, hipDeviceSynchronize()));
    return TRX_OK;
}

// Instance transforms: the TODOs at query_tlas.hlsl:409,433,484 and Traversable::get_instance_transform
// (traversable/src/lib.rs:25-27).  object_to_world: n column-major 4x4 matrices (glam Mat4) in TLAS-primitive order.
int trx_scene_set_instance_transforms(trx_scene *s, const float *object_to_world, uint32_t n) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    // The new table is built and uploaded first, the pointer is swapped under the launch mutex (enqueue() reads it
    // there, so no launch can pick up a table that is about to be freed), and the old table is freed only after
    // every kernel enqueued before the swap has drained.
    auto swap_table = [&](DevBuf<float4> fresh) -> int {
        DevBuf<float4> old;
        {
            std::lock_guard<std::mutex> lock(s->mu);
            old = std::move(s->inst_xform);
            s->inst_xform = std::move(fresh);
            s->emitters_stale = true; // (the emitter table holds world-space geometry)
            forget_tile_orders(s);
        }
        HIP_TRY(retire(old, hipDeviceSynchronize()));
        return TRX_OK;
    };
    if (!object_to_world || n == 0) { // back to identity
        const int rc = swap_table(DevBuf<float4>());
        if (rc) return rc;
        s->inst_o2w.clear();
        s->inst_w2o.clear();
        return TRX_OK;
    }
    if (!s->tlas) return fail(TRX_ERR_INVALID, "instance transforms need a TLAS scene");
    if (n != s->n_inst) return fail(TRX_ERR_INVALID, "%u transforms for %u instances", n, s->n_inst);
    std::vector<float> w2o((size_t)n * 12);
    for (uint32_t k = 0; k < n; k++) {
        const float *m = object_to_world + (size_t)k * 16; // m[c*4 + r]
        if (m[3] != 0.f || m[7] != 0.f || m[11] != 0.f || m[15] != 1.f)
            return fail(TRX_ERR_INVALID, "instance %u: transform is not affine (last row must be 0 0 0 1)", k);
        // inverse of the affine map in double, rounded once to f32
        const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
        const double tx = m[12], ty = m[13], tz = m[14];
        const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return fail(TRX_ERR_INVALID, "instance %u: singular transform", k);
        const double r = 1.0 / det;
        const double inv[9] = {(e * i - f * h) * r, (c * h - b * i) * r, (b * f - c * e) * r,
                               (f * g - d * i) * r, (a * i - c * g) * r, (c * d - a * f) * r,
                               (d * h - e * g) * r, (b * g - a * h) * r, (a * e - b * d) * r};
        float *o = &w2o[(size_t)k * 12];
        for (int row = 0; row < 3; row++) {
            o[4 * row + 0] = (float)inv[3 * row + 0];
            o[4 * row + 1] = (float)inv[3 * row + 1];
            o[4 * row + 2] = (float)inv[3 * row + 2];
            o[4 * row + 3] = (float)-(inv[3 * row + 0] * tx + inv[3 * row + 1] * ty + inv[3 * row + 2] * tz);
        }
    }
    DevBuf<float4> d;
    HIP_TRY(d.alloc(w2o.size() / 4));
    hipError_t e = hipMemcpy(d.get(), w2o.data(), w2o.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the instance transforms failed: %s", hipGetErrorString(e));
    const int rc_swap = swap_table(std::move(d));
    if (rc_swap) return rc_swap;
    s->inst_o2w.assign(object_to_world, object_to_world + (size_t)n * 16);
    s->inst_w2o.swap(w2o);
    return TRX_OK;
}

// Instance masks (include/trx.h): read by the masked trace calls only (enqueue() hands them the table under s->mu).
int trx_scene_set_instance_masks(trx_scene *s, const uint8_t *masks, uint32_t n) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (!s->tlas) return fail(TRX_ERR_INVALID, "instance masks need a TLAS scene");
    const bool remove = !masks || n == 0;
    if (!remove && n != s->n_inst) return fail(TRX_ERR_INVALID, "%u masks for %u instances", n, s->n_inst);
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint8_t> host_copy;
    DevBuf<uint8_t> fresh;
    if (!remove) {
        try {
            host_copy.assign(masks, masks + n);
        } catch (const std::exception &) {
            return fail(TRX_ERR_OOM, "host allocation failed");
        }
        HIP_TRY(fresh.alloc(n));
        const hipError_t e = hipMemcpy(fresh.get(), masks, n, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the instance masks failed: %s", hipGetErrorString(e));
    }
    // The pointer is swapped under the launch mutex (enqueue() reads it there), and the old table is freed once every
    // launch slot's last kernel has finished: a masked launch enqueued before this call uses the old table in full.  Slots
    // are waited for one by one - not the device, on which a resident kernel (a ray service) may be running - and
    // pinned slots are skipped: the resident kernels never read the table.
    DevBuf<uint8_t> old;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        old = std::move(s->inst_mask);
        s->inst_mask = std::move(fresh);
        s->h_inst_mask.swap(host_copy);
        if (old)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    if (retire(old, e) != hipSuccess) // (the old table is kept rather than freed under a kernel that may still read it)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

// Materials (include/trx.h, "materials"): read by the colour passes under s->mu, like the instance mask table.
int trx_scene_set_materials(trx_scene *s, const trx_material *materials, uint32_t n_materials, const uint16_t *tri_material,
                            uint64_t n_tris) {
    if (!s || !materials || !tri_material) return fail(TRX_ERR_INVALID, "null argument");
    if (n_materials == 0 || n_materials > TRX_MAX_MATERIALS)
        return fail(TRX_ERR_INVALID, "n_materials %u outside 1..%u", n_materials, TRX_MAX_MATERIALS);
    if (n_tris != s->n_tris)
        return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
    for (uint32_t m = 0; m < n_materials; m++)
        for (int c = 0; c < 3; c++) {
            const float a = materials[m].albedo[c], e = materials[m].emission[c];
            if (!std::isfinite(a) || a < 0.0f) return fail(TRX_ERR_INVALID, "material %u: albedo %g is negative or not finite", m, (double)a);
            if (!std::isfinite(e) || e < 0.0f) return fail(TRX_ERR_INVALID, "material %u: emission %g is negative or not finite", m, (double)e);
        }
    for (uint64_t i = 0; i < n_tris; i++)
        if (tri_material[i] >= n_materials)
            return fail(TRX_ERR_INVALID, "triangle %llu: material index %u of %u materials", (unsigned long long)i, (unsigned)tri_material[i], n_materials);
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<trx_material> host_mat;
    std::vector<uint16_t> host_idx;
    try {
        host_mat.assign(materials, materials + n_materials);
        host_idx.assign(tri_material, tri_material + n_tris);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    DevBuf<trx_material> fresh_mat;
    DevBuf<uint16_t> fresh_idx;
    HIP_TRY(fresh_mat.alloc(n_materials));
    HIP_TRY(fresh_idx.alloc(std::max<uint64_t>(n_tris, 1)));
    // (uploaded from the validated host copies: what the kernels index is what was checked)
    hipError_t e = hipMemcpy(fresh_mat.get(), host_mat.data(), (size_t)n_materials * sizeof(trx_material), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_tris) e = hipMemcpy(fresh_idx.get(), host_idx.data(), (size_t)n_tris * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the materials failed: %s", hipGetErrorString(e));
    // Swapped under the launch mutex (the colour passes read the pointers there); the old tables are freed once every launch
    // slot's last kernel has finished - trx_scene_set_instance_masks' statement: a pass enqueued before this call uses the
    // old tables in full.
    DevBuf<trx_material> old_mat;
    DevBuf<uint16_t> old_idx;
    TextureSet old_tex;
    e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        old_mat = std::move(s->materials);
        old_idx = std::move(s->tri_material);
        s->materials = std::move(fresh_mat);
        s->tri_material = std::move(fresh_idx);
        s->h_materials.swap(host_mat);
        s->h_tri_material.swap(host_idx);
        s->emitters_stale = true; // (the emitter table was chosen by, and indexes, the old materials)
        // (the texture set is keyed by material: one index per material of the table it was set for)
        if (s->material_texture && s->h_material_texture.size() != n_materials) old_tex.take_from(s);
        if (old_mat)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    (void)old_tex.retire_all(e);
    (void)retire(old_idx, e);
    if (retire(old_mat, e) != hipSuccess) // (the old tables are kept rather than freed under a kernel that may still read them)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_scene_get_materials(const trx_scene *s, trx_material *out_materials, uint32_t *inout_n_materials, uint16_t *out_tri_material,
                            uint64_t n_tris) {
    if (!s || !out_materials || !inout_n_materials || !out_tri_material) return fail(TRX_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (s->h_materials.empty()) return fail(TRX_ERR_INVALID, "the scene has no materials (trx_scene_set_materials)");
    if (n_tris != s->n_tris)
        return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
    if (*inout_n_materials < s->h_materials.size())
        return fail(TRX_ERR_INVALID, "room for %u materials, the scene has %zu", *inout_n_materials, s->h_materials.size());
    std::memcpy(out_materials, s->h_materials.data(), s->h_materials.size() * sizeof(trx_material));
    if (n_tris) std::memcpy(out_tri_material, s->h_tri_material.data(), (size_t)n_tris * sizeof(uint16_t));
    *inout_n_materials = (uint32_t)s->h_materials.size();
    return TRX_OK;
}

// Vertex normals (include/trx.h, "vertex normals"): read by the shading-normal pass under s->mu, owned like the materials.
int trx_scene_set_vertex_normals(trx_scene *s, const float *normals, uint64_t n_tris) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    const bool remove = !normals || n_tris == 0;
    if (!remove) {
        if (n_tris != s->n_tris)
            return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
        for (uint64_t i = 0; i < n_tris * 9; i++)
            if (!std::isfinite(normals[i]))
                return fail(TRX_ERR_INVALID, "triangle %llu: vertex normal component %g is not finite", (unsigned long long)(i / 9), (double)normals[i]);
    }
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<float> host_copy;
    DevBuf<float4> fresh;
    if (!remove) {
        std::vector<float> padded; // three float4 per triangle, w = +0
        try {
            host_copy.assign(normals, normals + n_tris * 9);
            padded.assign((size_t)n_tris * 12, 0.0f);
        } catch (const std::exception &) {
            return fail(TRX_ERR_OOM, "host allocation failed");
        }
        for (uint64_t i = 0; i < n_tris * 3; i++)
            for (int c = 0; c < 3; c++) padded[i * 4 + c] = host_copy[i * 3 + c];
        HIP_TRY(fresh.alloc(n_tris * 3));
        // (uploaded from the validated host copy)
        const hipError_t e = hipMemcpy(fresh.get(), padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the vertex normals failed: %s", hipGetErrorString(e));
    }
    // Swapped under the launch mutex (the shading-normal pass reads the pointer there); the old table is freed once every
    // launch slot's last kernel has finished - trx_scene_set_instance_masks' statement: a pass enqueued before this call uses
    // the old table in full.
    DevBuf<float4> old;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        old = std::move(s->vertex_normals);
        s->vertex_normals = std::move(fresh);
        s->h_vertex_normals.swap(host_copy);
        if (old)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    if (retire(old, e) != hipSuccess) // (the old table is kept rather than freed under a kernel that may still read it)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_scene_get_vertex_normals(const trx_scene *s, float *out_normals, uint64_t n_tris) {
    if (!s || !out_normals) return fail(TRX_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (!s->vertex_normals) return fail(TRX_ERR_INVALID, "the scene has no vertex normals (trx_scene_set_vertex_normals)");
    if (n_tris != s->n_tris)
        return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
    if (n_tris) std::memcpy(out_normals, s->h_vertex_normals.data(), (size_t)n_tris * 9 * sizeof(float));
    return TRX_OK;
}

// Texture coordinates (include/trx.h, "texture coordinates and albedo textures"): read by the albedo pass under s->mu, owned
// like the vertex normals.  Any float is legal: the sampling rule handles what is not finite.
int trx_scene_set_texcoords(trx_scene *s, const float *uvs, uint64_t n_tris) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    const bool remove = !uvs || n_tris == 0;
    if (!remove && n_tris != s->n_tris)
        return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<float> host_copy;
    DevBuf<float2> fresh;
    if (!remove) {
        try {
            host_copy.assign(uvs, uvs + n_tris * 6);
        } catch (const std::exception &) {
            return fail(TRX_ERR_OOM, "host allocation failed");
        }
        HIP_TRY(fresh.alloc(n_tris * 3));
        const hipError_t e = hipMemcpy(fresh.get(), host_copy.data(), host_copy.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the texture coordinates failed: %s", hipGetErrorString(e));
    }
    // Swapped under the launch mutex (the albedo pass reads the pointer there); the old table is freed once every launch
    // slot's last kernel has finished - trx_scene_set_instance_masks' statement.
    DevBuf<float2> old;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        old = std::move(s->texcoords);
        s->texcoords = std::move(fresh);
        s->h_texcoords.swap(host_copy);
        if (old)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    if (retire(old, e) != hipSuccess) // (the old table is kept rather than freed under a kernel that may still read it)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_scene_get_texcoords(const trx_scene *s, float *out_uvs, uint64_t n_tris) {
    if (!s || !out_uvs) return fail(TRX_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (!s->texcoords) return fail(TRX_ERR_INVALID, "the scene has no texture coordinates (trx_scene_set_texcoords)");
    if (n_tris != s->n_tris)
        return fail(TRX_ERR_INVALID, "n_tris %llu: the scene has %llu triangles", (unsigned long long)n_tris, (unsigned long long)s->n_tris);
    if (n_tris) std::memcpy(out_uvs, s->h_texcoords.data(), (size_t)n_tris * 6 * sizeof(float));
    return TRX_OK;
}

void trx_texture_srgb_table(float out[256]) {
    if (!out) return;
    for (int c = 0; c < 256; c++) {
        const double x = (double)c / 255.0;
        out[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4));
    }
}

// The texture set (include/trx.h, "THE TEXTURE SET"): everything a kernel will index is checked here, on the host, before
// anything is copied; the four device tables are swapped together under s->mu and owned like the materials.
int trx_scene_set_textures(trx_scene *s, const trx_texture_desc *descs, uint32_t n_textures, const uint32_t *texels, uint64_t n_texels,
                           const uint32_t *material_texture, uint32_t n_materials) {
    if (!s || !descs || !texels || !material_texture) return fail(TRX_ERR_INVALID, "null argument");
    if (n_textures == 0 || n_textures > TRX_MAX_TEXTURES) return fail(TRX_ERR_INVALID, "n_textures %u outside 1..%u", n_textures, TRX_MAX_TEXTURES);
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_textures; k++) {
        const trx_texture_desc &d = descs[k];
        if (d.width == 0 || d.width > TRX_MAX_TEXTURE_SIZE || d.height == 0 || d.height > TRX_MAX_TEXTURE_SIZE)
            return fail(TRX_ERR_INVALID, "texture %u: %u x %u texels outside 1..%u", k, d.width, d.height, TRX_MAX_TEXTURE_SIZE);
        if (d.format != TRX_TEX_RGBA8_UNORM && d.format != TRX_TEX_RGBA8_SRGB) return fail(TRX_ERR_INVALID, "texture %u: unknown format %u", k, d.format);
        if (d.filter != TRX_TEX_NEAREST && d.filter != TRX_TEX_BILINEAR) return fail(TRX_ERR_INVALID, "texture %u: unknown filter %u", k, d.filter);
        sum += (uint64_t)d.width * d.height; // (at most 65535 * 2^26: no overflow)
    }
    if (n_texels != sum) return fail(TRX_ERR_INVALID, "n_texels %llu: the descriptors hold %llu texels", (unsigned long long)n_texels, (unsigned long long)sum);
    if (n_texels >= 0x80000000ull) return fail(TRX_ERR_INVALID, "n_texels %llu: beyond 2^31 - 1", (unsigned long long)n_texels);
    for (uint32_t m = 0; m < n_materials; m++)
        if (material_texture[m] != TRX_NO_TEXTURE && material_texture[m] >= n_textures)
            return fail(TRX_ERR_INVALID, "material %u: texture index %u of %u textures", m, material_texture[m], n_textures);
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (trx_scene_set_materials holds it too: the count below stays)
    {
        std::lock_guard<std::mutex> lock(s->mu);
        if (s->h_materials.empty()) return fail(TRX_ERR_INVALID, "the scene has no materials (trx_scene_set_materials)");
        if (n_materials != s->h_materials.size())
            return fail(TRX_ERR_INVALID, "n_materials %u: the scene has %zu materials", n_materials, s->h_materials.size());
    }
    HIP_TRY(hipSetDevice(s->device));
    TextureSet fresh;
    std::vector<uint4> dev_descs;
    float srgb[256];
    trx_texture_srgb_table(srgb);
    try {
        fresh.h_descs.assign(descs, descs + n_textures);
        fresh.h_texels.assign(texels, texels + n_texels);
        fresh.h_material_texture.assign(material_texture, material_texture + n_materials);
        dev_descs.resize(n_textures);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    uint32_t offset = 0;
    for (uint32_t k = 0; k < n_textures; k++) {
        const trx_texture_desc &d = fresh.h_descs[k];
        dev_descs[k] = make_uint4(offset, d.width, d.height, d.format | d.filter << 8);
        offset += d.width * d.height;
    }
    HIP_TRY(fresh.descs.alloc(n_textures));
    HIP_TRY(fresh.texels.alloc(n_texels));
    HIP_TRY(fresh.material_texture.alloc(n_materials));
    HIP_TRY(fresh.srgb.alloc(256));
    // (uploaded from the validated host copies: what the kernels index is what was checked)
    hipError_t e = hipMemcpy(fresh.descs.get(), dev_descs.data(), (size_t)n_textures * sizeof(uint4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fresh.texels.get(), fresh.h_texels.data(), (size_t)n_texels * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(fresh.material_texture.get(), fresh.h_material_texture.data(), (size_t)n_materials * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fresh.srgb.get(), srgb, sizeof(srgb), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "upload of the textures failed: %s", hipGetErrorString(e));
    TextureSet old;
    e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        const bool had = (bool)s->material_texture;
        old.take_from(s);
        fresh.give_to(s);
        if (had)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    if (old.retire_all(e) != hipSuccess) // (the old set is kept rather than freed under a kernel that may still read it)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_scene_remove_textures(trx_scene *s) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    TextureSet old;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        const bool had = (bool)s->material_texture;
        old.take_from(s);
        if (had)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    if (old.retire_all(e) != hipSuccess)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_scene_get_textures(const trx_scene *s, trx_texture_desc *out_descs, uint32_t *inout_n_textures, uint32_t *out_texels,
                           uint64_t *inout_n_texels, uint32_t *out_material_texture, uint32_t *inout_n_materials) {
    if (!s || !out_descs || !inout_n_textures || !out_texels || !inout_n_texels || !out_material_texture || !inout_n_materials)
        return fail(TRX_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (!s->material_texture) return fail(TRX_ERR_INVALID, "the scene has no textures (trx_scene_set_textures)");
    const bool room = *inout_n_textures >= s->h_tex_descs.size() && *inout_n_texels >= s->h_texels.size() &&
                      *inout_n_materials >= s->h_material_texture.size();
    *inout_n_textures = (uint32_t)s->h_tex_descs.size();
    *inout_n_texels = s->h_texels.size();
    *inout_n_materials = (uint32_t)s->h_material_texture.size();
    if (!room)
        return fail(TRX_ERR_INVALID, "too little room: the scene has %u textures, %llu texels, %u materials", *inout_n_textures,
                    (unsigned long long)*inout_n_texels, *inout_n_materials);
    std::memcpy(out_descs, s->h_tex_descs.data(), s->h_tex_descs.size() * sizeof(trx_texture_desc));
    std::memcpy(out_texels, s->h_texels.data(), s->h_texels.size() * sizeof(uint32_t));
    std::memcpy(out_material_texture, s->h_material_texture.data(), s->h_material_texture.size() * sizeof(uint32_t));
    return TRX_OK;
}

int trx_scene_get_instance_masks(const trx_scene *s, uint8_t *out, uint32_t n) {
    if (!s || (!out && n)) return fail(TRX_ERR_INVALID, "null argument");
    const uint32_t want = s->tlas ? s->n_inst : 1u; // (a single-level scene is one instance with mask 0xFF)
    if (n != want) return fail(TRX_ERR_INVALID, "%u masks asked for %u instances", n, want);
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (s->h_inst_mask.empty()) std::memset(out, 0xff, n);
    else std::memcpy(out, s->h_inst_mask.data(), n);
    return TRX_OK;
}

int trx_scene_get_instance_transform(const trx_scene *s, uint32_t instance_id, float out_object_to_world[16]) {
    if (!s || !out_object_to_world) return fail(TRX_ERR_INVALID, "null argument");
    if (instance_id >= std::max<uint32_t>(s->n_inst, 1)) return fail(TRX_ERR_INVALID, "instance %u of %u", instance_id, s->n_inst);
    if (s->inst_o2w.empty()) { // Mat4::default(): identity, like the reference (src/cwbvh.rs:163-165,189-191)
        for (int k = 0; k < 16; k++) out_object_to_world[k] = (k % 5 == 0) ? 1.f : 0.f;
        return TRX_OK;
    }
    std::memcpy(out_object_to_world, &s->inst_o2w[(size_t)instance_id * 16], 64);
    return TRX_OK;
}

int trx_scene_get_instance_world_to_object(const trx_scene *s, uint32_t instance_id, float out_rows[12]) {
    if (!s || !out_rows) return fail(TRX_ERR_INVALID, "null argument");
    if (instance_id >= std::max<uint32_t>(s->n_inst, 1)) return fail(TRX_ERR_INVALID, "instance %u of %u", instance_id, s->n_inst);
    if (s->inst_w2o.empty()) {
        static const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        std::memcpy(out_rows, ident, 48);
        return TRX_OK;
    }
    std::memcpy(out_rows, &s->inst_w2o[(size_t)instance_id * 12], 48);
    return TRX_OK;
}

// ---- camera: ViewUniform::from_camera, src/main.rs:602-616 -----------------------------
static void mat4_inverse_f32(const float m[16], float out[16]) {
    // cofactor expansion (same scheme as glam's Mat4::inverse), evaluated in f32
    const float a00 = m[0], a01 = m[1], a02 = m[2], a03 = m[3], a10 = m[4], a11 = m[5], a12 = m[6], a13 = m[7];
    const float a20 = m[8], a21 = m[9], a22 = m[10], a23 = m[11], a30 = m[12], a31 = m[13], a32 = m[14], a33 = m[15];
    const float b00 = a00 * a11 - a01 * a10, b01 = a00 * a12 - a02 * a10, b02 = a00 * a13 - a03 * a10;
    const float b03 = a01 * a12 - a02 * a11, b04 = a01 * a13 - a03 * a11, b05 = a02 * a13 - a03 * a12;
    const float b06 = a20 * a31 - a21 * a30, b07 = a20 * a32 - a22 * a30, b08 = a20 * a33 - a23 * a30;
    const float b09 = a21 * a32 - a22 * a31, b10 = a21 * a33 - a23 * a31, b11 = a22 * a33 - a23 * a32;
    const float det = b00 * b11 - b01 * b10 + b02 * b09 + b03 * b08 - b04 * b07 + b05 * b06;
    const float r = 1.0f / det;
    out[0] = (a11 * b11 - a12 * b10 + a13 * b09) * r;
    out[1] = (a02 * b10 - a01 * b11 - a03 * b09) * r;
    out[2] = (a31 * b05 - a32 * b04 + a33 * b03) * r;
    out[3] = (a22 * b04 - a21 * b05 - a23 * b03) * r;
    out[4] = (a12 * b08 - a10 * b11 - a13 * b07) * r;
    out[5] = (a00 * b11 - a02 * b08 + a03 * b07) * r;
    out[6] = (a32 * b02 - a30 * b05 - a33 * b01) * r;
    out[7] = (a20 * b05 - a22 * b02 + a23 * b01) * r;
    out[8] = (a10 * b10 - a11 * b08 + a13 * b06) * r;
    out[9] = (a01 * b08 - a00 * b10 - a03 * b06) * r;
    out[10] = (a30 * b04 - a31 * b02 + a33 * b00) * r;
    out[11] = (a21 * b02 - a20 * b04 - a23 * b00) * r;
    out[12] = (a11 * b07 - a10 * b09 - a12 * b06) * r;
    out[13] = (a00 * b09 - a01 * b07 + a02 * b06) * r;
    out[14] = (a31 * b01 - a30 * b03 - a32 * b00) * r;
    out[15] = (a20 * b03 - a21 * b01 + a22 * b00) * r;
}

int trx_view_from_camera(const float eye[3], const float look_at[3], float fov_deg, float width, float height,
                         trx_view *out) {
    if (!eye || !look_at || !out) return fail(TRX_ERR_INVALID, "null argument");
    if (!(width > 0.f) || !(height > 0.f)) return fail(TRX_ERR_INVALID, "bad image size");
    std::memset(out, 0, sizeof(*out));
    const float aspect = width / height;
    const float fov = fov_deg * (3.14159265358979323846f / 180.0f);
    const float f = 1.0f / std::tan(0.5f * fov);
    float proj[16] = {0};
    proj[0] = f / aspect;
    proj[5] = f;
    proj[11] = -1.0f;
    proj[14] = 0.01f;
    mat4_inverse_f32(proj, out->proj_inv);
    float fw[3] = {look_at[0] - eye[0], look_at[1] - eye[1], look_at[2] - eye[2]};
    float fl = std::sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]);
    if (!(fl > 0.f)) return fail(TRX_ERR_INVALID, "eye == look_at");
    for (float &x : fw) x /= fl;
    // s = normalize(f x up), up = +Y
    float s[3] = {fw[1] * 0.f - fw[2] * 1.f, fw[2] * 0.f - fw[0] * 0.f, fw[0] * 1.f - fw[1] * 0.f};
    float sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (!(sl > 0.f)) return fail(TRX_ERR_INVALID, "view direction parallel to +Y");
    for (float &x : s) x /= sl;
    float u[3] = {s[1] * fw[2] - s[2] * fw[1], s[2] * fw[0] - s[0] * fw[2], s[0] * fw[1] - s[1] * fw[0]};
    auto dot = [](const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    float view[16] = {s[0], u[0], -fw[0], 0, s[1], u[1], -fw[1], 0, s[2], u[2], -fw[2], 0,
                      -dot(s, eye), -dot(u, eye), dot(fw, eye), 1};
    mat4_inverse_f32(view, out->view_inv);
    std::memcpy(out->eye, eye, 12);
    return TRX_OK;
}

} // extern "C"
