// api_attr.cpp - hit attributes (include/trx.h, trx_hit_attr): the post-pass that turns hit records into the barycentrics
// and the world-space geometric normal of the committed triangle test (k_hit_attr, kernels.hip).  Its launches take a
// launch slot of the scene like the traversal kernels do, so trx_scene_refit waits for them.  The shading-normal pass
// (trx_shading_normals_*, k_shading_normal) rewrites the normal of such records from the scene's vertex normals the same way.
#include "api_internal.h"

namespace {

// One k_hit_attr pass over p.n_items records (split into launches of at most 2^30 for rays), on a launch slot.
int enqueue_attr(trx_scene *s, HitAttrParams &p, int mode, uint64_t n, const uint32_t *d_inst, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    const bool xf = s->tlas && s->inst_xform;
    if (xf && !d_inst)
        return fail(TRX_ERR_INVALID, "this scene has instance transforms: the attribute pass needs the instance id of every "
                                     "hit (the trace's d_inst) to take the ray into object space and the normal to world space");
    if (n == 0) return TRX_OK;
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    p.tris = s->tris.get();
    p.inst_xform = xf ? s->inst_xform.get() : nullptr;
    p.inst = xf ? d_inst : nullptr;
    p.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull);
    p.n_inst = s->n_inst;
    slot->last_stream = stream;
    slot->last_use = ++s->launches;
    if (mode == kAttrRays) {
        const uint64_t chunk = 1ull << 30;
        const HitAttrParams base = p;
        for (uint64_t off = 0; off < n; off += chunk) {
            p = base;
            p.rays = base.rays + off;
            p.hits = base.hits + off;
            p.inst = base.inst ? base.inst + off : nullptr;
            p.out = base.out + off;
            p.n_items = (uint32_t)std::min(chunk, n - off);
            HIP_TRY(launch_hit_attr(p, mode, stream));
        }
    } else {
        HIP_TRY(launch_hit_attr(p, mode, stream));
    }
    HIP_TRY(hipEventRecord(slot->done.get(), stream));
    slot->used = true;
    return TRX_OK;
}

// One k_shading_normal pass over p.n_items records, on a launch slot exactly as enqueue_attr takes one: a refit or a swap of
// the vertex-normal table called afterwards waits for the slot's `done` event.
int enqueue_shading_normal(trx_scene *s, ShadingNormalParams &p, int mode, uint64_t n, const uint32_t *d_inst, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->vertex_normals) return fail(TRX_ERR_INVALID, "the scene has no vertex normals (trx_scene_set_vertex_normals)");
    const bool xf = s->tlas && s->inst_xform;
    if (xf && !d_inst)
        return fail(TRX_ERR_INVALID, "this scene has instance transforms: the shading-normal pass needs the instance id of every "
                                     "hit (the trace's d_inst) to take the vertex normals to world space");
    if (n == 0) return TRX_OK;
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    p.normals = s->vertex_normals.get();
    p.inst_xform = xf ? s->inst_xform.get() : nullptr;
    p.inst = xf ? d_inst : nullptr;
    p.n_tris = (uint32_t)std::min<uint64_t>(s->vertex_normals.count() / 3, 0xffffffffull);
    p.n_inst = s->n_inst;
    slot->last_stream = stream;
    slot->last_use = ++s->launches;
    if (mode == kAttrRays) {
        const uint64_t chunk = 1ull << 30;
        const ShadingNormalParams base = p;
        for (uint64_t off = 0; off < n; off += chunk) {
            p = base;
            p.rays = base.rays + off;
            p.hits = base.hits + off;
            p.inst = base.inst ? base.inst + off : nullptr;
            p.attr = base.attr + off;
            p.out = base.out + off;
            p.n_items = (uint32_t)std::min(chunk, n - off);
            HIP_TRY(launch_shading_normal(p, mode, stream));
        }
    } else {
        HIP_TRY(launch_shading_normal(p, mode, stream));
    }
    HIP_TRY(hipEventRecord(slot->done.get(), stream));
    slot->used = true;
    return TRX_OK;
}

} // namespace

extern "C" {

int trx_hit_attributes_rays_dev(trx_scene *s, const trx_ray *d_rays, uint64_t n, const trx_hit *d_hits,
                                const uint32_t *d_inst, trx_hit_attr *d_attr, void *stream) {
    if (!s || (n && (!d_rays || !d_hits || !d_attr))) return fail(TRX_ERR_INVALID, "null argument");
    HitAttrParams p;
    std::memset(&p, 0, sizeof(p));
    p.rays = d_rays;
    p.hits = d_hits;
    p.out = d_attr;
    return enqueue_attr(s, p, kAttrRays, n, d_inst, (hipStream_t)stream);
}

int trx_hit_attributes_primary_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard,
                                   const trx_hit *d_hits, const uint32_t *d_inst, trx_hit_attr *d_attr, void *stream) {
    if (!s || !d_hits || !d_attr) return fail(TRX_ERR_INVALID, "null argument");
    TraceParams t; // (the image geometry exactly as the trace derives it)
    int rc = image_params(t, view, w, h, shard);
    if (rc) return rc;
    HitAttrParams p;
    std::memset(&p, 0, sizeof(p));
    p.hits = d_hits;
    p.out = d_attr;
    p.n_items = t.n_items;
    p.geom = tile_geom(t);
    p.view = t.views[0];
    return enqueue_attr(s, p, kAttrPrimary, t.n_items, d_inst, (hipStream_t)stream);
}

int trx_shading_normals_rays_dev(trx_scene *s, const trx_ray *d_rays, uint64_t n, const trx_hit *d_hits, const uint32_t *d_inst,
                                 const trx_hit_attr *d_attr, trx_hit_attr *d_out, void *stream) {
    if (!s || (n && (!d_rays || !d_hits || !d_attr || !d_out))) return fail(TRX_ERR_INVALID, "null argument");
    ShadingNormalParams p;
    std::memset(&p, 0, sizeof(p));
    p.rays = d_rays;
    p.hits = d_hits;
    p.attr = d_attr;
    p.out = d_out;
    return enqueue_shading_normal(s, p, kAttrRays, n, d_inst, (hipStream_t)stream);
}

int trx_shading_normals_primary_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, const trx_hit *d_hits,
                                    const uint32_t *d_inst, const trx_hit_attr *d_attr, trx_hit_attr *d_out, void *stream) {
    if (!s || !d_hits || !d_attr || !d_out) return fail(TRX_ERR_INVALID, "null argument");
    TraceParams t; // (the image geometry exactly as the trace derives it)
    int rc = image_params(t, view, w, h, shard);
    if (rc) return rc;
    ShadingNormalParams p;
    std::memset(&p, 0, sizeof(p));
    p.hits = d_hits;
    p.attr = d_attr;
    p.out = d_out;
    p.n_items = t.n_items;
    p.geom = tile_geom(t);
    p.view = t.views[0];
    return enqueue_shading_normal(s, p, kAttrPrimary, t.n_items, d_inst, (hipStream_t)stream);
}

int trx_trace_rays_attr(trx_scene *s, const trx_ray *rays, uint64_t n, uint32_t sem, trx_hit *out_hits, uint32_t *out_inst,
                        trx_hit_attr *out_attr, float *out_ms) {
    if (!s || (n && !rays)) return fail(TRX_ERR_INVALID, "null argument");
    if (n == 0) return TRX_OK;
    // (two-level scenes always trace the instance ids: the attribute pass needs them under instance transforms)
    auto d_inst = [&] { return s->tlas ? s->scratch_ia.get() : nullptr; };
    return host_call(
        s, n, rays, n, n, out_ms,
        [&] {
            int rc = trx_trace_rays_inst_dev(s, s->scratch_rays.get(), n, sem, s->scratch_a.get(), d_inst(), nullptr);
            if (rc) return rc;
            return trx_hit_attributes_rays_dev(s, s->scratch_rays.get(), n, s->scratch_a.get(), d_inst(), s->scratch_attr.get(), nullptr);
        },
        [&]() -> int {
            if (out_hits) HIP_TRY(hipMemcpy(out_hits, s->scratch_a.get(), n * sizeof(trx_hit), hipMemcpyDeviceToHost));
            if (int rc = read_inst(out_inst, d_inst(), n)) return rc;
            if (out_attr) HIP_TRY(hipMemcpy(out_attr, s->scratch_attr.get(), n * sizeof(trx_hit_attr), hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

} // extern "C"
