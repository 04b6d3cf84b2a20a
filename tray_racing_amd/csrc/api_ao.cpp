// api_ao.cpp - AO visibility (include/trx.h, trx_ao_rays_dev / trx_trace_ao_visibility* / trx_trace_ao_visibility_sparse_dev): the AO pass's rays written out as
// explicit rays (k_ao_rays, kernels.hip), walked by the any-hit rays launch every trx_trace_occluded*_dev call uses, and
// their flags added into one count per pixel (k_ao_reduce).  A composition around the shipped walk: no traversal kernel
// knows about it.  Everything of one call runs on the caller's stream, on that stream's launch slot of the scene - the slot
// owns the ray scratch, so concurrent calls on other streams have their own - and trx_scene_refit waits for it like for any
// other launch of the slot.  The sparse pass is the same chain over the tiles of a low grid whose cells name every
// stride-th pixel of the full image (kernels.h, AoRaysParams): same scratch, same cap, same chunk loops.
#include "api_internal.h"

#include <cfloat>

namespace {

// The scratch of one launch slot holds at most this many bytes of rays and flags (kAoUnitBytes per tile and sample): the
// four-sample 1080p pass (32 400 tiles x 4 x 2 112 B = 261 MiB) is one chunk, anything larger runs in several.
constexpr uint64_t kAoScratchCapDefault = 288ull << 20;
std::atomic<uint64_t> g_ao_scratch_cap{kAoScratchCapDefault};

// ao_radius -> the rays' tmax: > 0, +inf stored as FLT_MAX (what the AO pass walks to)
int radius_tmax(float ao_radius, float &tmax) {
    if (!(ao_radius > 0.0f)) return fail(TRX_ERR_INVALID, "ao_radius %g: must be > 0 (+inf allowed)", (double)ao_radius);
    tmax = ao_radius > FLT_MAX ? FLT_MAX : ao_radius;
    return TRX_OK;
}

// the image geometry exactly as the trace derives it, and what both kernels need of the scene (s->mu held for the scene part)
int ao_geometry(AoRaysParams &p, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t &tiles) {
    TraceParams t;
    if (int rc = image_params(t, view, w, h, shard)) return rc;
    std::memset(&p, 0, sizeof(p));
    p.geom = tile_geom(t);
    p.view = t.views[0];
    tiles = t.tiles_per_frame;
    return TRX_OK;
}

int need_inst(const trx_scene *s, const uint32_t *d_primary_inst) {
    if (s->tlas && s->inst_xform && !d_primary_inst)
        return fail(TRX_ERR_INVALID, "this scene has instance transforms: the AO rays need the primary pass's instance ids "
                                     "(d_primary_inst) to take the hit normal into world space");
    return TRX_OK;
}

// the sparse pass's grid: cell (X, Y) of the ceil(w / stride) x ceil(h / stride) low grid is pixel (X * stride + px0, Y * stride + py0)
struct SparseGrid {
    uint32_t stride, phase;
};
int check_sparse(uint32_t stride, uint32_t phase) {
    if (stride == 0 || stride > TRX_MAX_AO_STRIDE) return fail(TRX_ERR_INVALID, "stride %u outside 1..%d", stride, TRX_MAX_AO_STRIDE);
    if (phase >= stride * stride) return fail(TRX_ERR_INVALID, "phase %u outside 0..%u (stride %u)", phase, stride * stride - 1, stride);
    return TRX_OK;
}

// hipEvents around the three phases of every chunk (trx_debug_ao_visibility_phases)
struct Phases {
    std::vector<Event> ev; // 4 per chunk: before the rays, after them, after the walk, after the reduce
    int mark(hipStream_t stream) {
        ev.emplace_back();
        HIP_TRY(ev.back().create());
        HIP_TRY(hipEventRecord(ev.back().get(), stream));
        return TRX_OK;
    }
};

int visibility_impl(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t frame0,
                    uint32_t n_samples, float ao_eps, float ao_radius, const trx_hit *d_primary,
                    const uint32_t *d_primary_inst, uint8_t *d_unoccluded, hipStream_t stream, Phases *phases,
                    const SparseGrid *sparse = nullptr) {
    if (!s || !d_primary || !d_unoccluded) return fail(TRX_ERR_INVALID, "null argument");
    if (sparse) if (int rc = check_sparse(sparse->stride, sparse->phase)) return rc;
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    AoRaysParams g;
    uint32_t tiles = 0;
    float tmax = 0.f;
    if (int rc = radius_tmax(ao_radius, tmax)) return rc;
    if (int rc = ao_geometry(g, view, w, h, shard, tiles)) return rc;
    if (sparse) {
        // (the full image's geometry stays in g.geom and g.view: the rays are its rays; the tiles are the low grid's)
        AoRaysParams lo;
        const uint32_t st = sparse->stride;
        if (int rc = ao_geometry(lo, view, (w + st - 1) / st, (h + st - 1) / st, shard, tiles)) return rc;
        g.lo = lo.geom;
        g.stride = st;
        g.px0 = sparse->phase % st;
        g.py0 = sparse->phase / st;
    }
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    // chunks: as many tiles as the scratch holds, and for them as many samples as it holds
    const uint64_t units = std::min<uint64_t>(std::max<uint64_t>(g_ao_scratch_cap.load(std::memory_order_relaxed) / kAoUnitBytes, 1), 1ull << 24);
    const uint32_t tile_chunk = (uint32_t)std::min<uint64_t>(tiles, units);
    const uint32_t sample_chunk = (uint32_t)std::min<uint64_t>(n_samples, std::max<uint64_t>(units / tile_chunk, 1));
    const uint64_t rays = (uint64_t)tile_chunk * sample_chunk * 64;
    if (slot->ao_rays.count() < rays) {
        // (the slot's previous kernel may still be walking the old scratch)
        if (slot->used) HIP_TRY(hipEventSynchronize(slot->done.get()));
        slot->ao_flags.reset();
        HIP_TRY(slot->ao_rays.alloc(rays));
        HIP_TRY(slot->ao_flags.alloc(rays));
    }
    g.tris = s->tris.get();
    g.inst_xform = s->tlas ? s->inst_xform.get() : nullptr;
    g.primary = d_primary;
    g.primary_inst = g.inst_xform ? d_primary_inst : nullptr;
    g.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull); // (kernels.h, surface_record)
    g.n_inst = s->n_inst;
    g.rays = slot->ao_rays.get();
    g.flags = slot->ao_flags.get();
    g.counts = d_unoccluded;
    g.scratch = 1u;
    g.ao_eps = ao_eps;
    g.tmax = tmax;
    for (uint32_t tile0 = 0; tile0 < tiles; tile0 += tile_chunk) {
        for (uint32_t s0 = 0; s0 < n_samples; s0 += sample_chunk) {
            g.tile0 = tile0;
            g.n_tiles = std::min(tile_chunk, tiles - tile0);
            g.n_samples = std::min(sample_chunk, n_samples - s0);
            g.frame = frame0 + s0;
            g.first = s0 == 0 ? 1u : 0u;
            if (phases) if (int rc = phases->mark(stream)) return rc;
            HIP_TRY(launch_ao_rays(g, stream));
            // (from here on the slot is this stream's: the rays launch below finds it by its stream)
            slot->last_stream = stream;
            slot->last_use = ++s->launches;
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            slot->used = true;
            if (phases) if (int rc = phases->mark(stream)) return rc;
            TraceParams p;
            std::memset(&p, 0, sizeof(p));
            p.rays = g.rays;
            p.out = reinterpret_cast<trx_hit *>(slot->ao_flags.get());
            p.any_hit = 1u;
            p.n_items = g.n_tiles * g.n_samples * 64u;
            SlotCounters *ctr = nullptr;
            if (int rc = enqueue_locked(s, p, kModeRays, sem, false, stream, &ctr)) return rc;
            if (ctr != slot->ctr.get()) return fail(TRX_ERR_INVALID, "internal: the rays launch left the pass's launch slot");
            if (phases) if (int rc = phases->mark(stream)) return rc;
            HIP_TRY(launch_ao_reduce(g, stream));
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            if (phases) if (int rc = phases->mark(stream)) return rc;
        }
    }
    return TRX_OK;
}


// ---- direct light (include/trx.h, "direct light"): the pass above once per light, with a ray mask ----------------------------

int check_eps(float shadow_eps) {
    if (!(shadow_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "shadow_eps %g: must be >= 0", (double)shadow_eps);
    return TRX_OK;
}

void light_scene(LightRaysParams &g, const trx_scene *s, const trx_hit *d_primary, const uint32_t *d_primary_inst) {
    g.tris = s->tris.get();
    g.inst_xform = s->tlas ? s->inst_xform.get() : nullptr;
    g.primary = d_primary;
    g.primary_inst = g.inst_xform ? d_primary_inst : nullptr;
    g.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull); // (kernels.h, surface_record)
    g.n_inst = s->n_inst;
}

// visibility_impl's sibling: its chunk loops and slot bookkeeping statement for statement, per light, with k_light_rays /
// k_light_reduce around the rays launch and p.ray_mask set.  The AO pass's own path is left as it was.
int light_visibility_impl(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                          const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float shadow_eps,
                          const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_lit, hipStream_t stream, Phases *phases) {
    if (!s || !d_primary || !d_lit) return fail(TRX_ERR_INVALID, "null argument");
    if (int rc = check_lights(lights, n_lights, n_samples)) return rc;
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (ray_mask > 0xffu) return fail(TRX_ERR_INVALID, "ray_mask 0x%x outside 0..255", ray_mask);
    if (int rc = check_eps(shadow_eps)) return rc;
    AoRaysParams geom;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(geom, view, w, h, shard, tiles)) return rc;
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    if (tiles == 0) return TRX_OK;
    const uint64_t records = geom.geom.compact ? (uint64_t)tiles * 64u : (uint64_t)w * h;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    LightRaysParams g;
    std::memset(&g, 0, sizeof(g));
    g.geom = geom.geom;
    g.view = geom.view;
    light_scene(g, s, d_primary, d_primary_inst);
    g.scratch = 1u;
    g.shadow_eps = shadow_eps;
    // chunks: as many tiles as the scratch holds, and for them as many samples as it holds; the scratch is sized once, for the
    // light with the most samples
    const uint64_t units = std::min<uint64_t>(std::max<uint64_t>(g_ao_scratch_cap.load(std::memory_order_relaxed) / kAoUnitBytes, 1), 1ull << 24);
    const uint32_t tile_chunk = (uint32_t)std::min<uint64_t>(tiles, units);
    auto samples_of = [&](const trx_light &l) { return l.kind == TRX_LIGHT_RECT ? n_samples : 1u; }; // (one ray per pixel reaches a point or a direction)
    auto sample_chunk_of = [&](uint32_t n_k) { return (uint32_t)std::min<uint64_t>(n_k, std::max<uint64_t>(units / tile_chunk, 1)); };
    uint32_t most = 1u;
    for (uint32_t k = 0; k < n_lights; k++) most = std::max(most, samples_of(lights[k]));
    const uint64_t rays = (uint64_t)tile_chunk * sample_chunk_of(most) * 64;
    if (slot->ao_rays.count() < rays) {
        // (the slot's previous kernel may still be walking the old scratch)
        if (slot->used) HIP_TRY(hipEventSynchronize(slot->done.get()));
        slot->ao_flags.reset();
        HIP_TRY(slot->ao_rays.alloc(rays));
        HIP_TRY(slot->ao_flags.alloc(rays));
    }
    for (uint32_t k = 0; k < n_lights; k++) {
        const uint32_t n_k = samples_of(lights[k]), sample_chunk = sample_chunk_of(n_k);
        g.rays = slot->ao_rays.get();
        g.flags = slot->ao_flags.get();
        g.counts = d_lit + k * records;
        g.light = lights[k];
        for (uint32_t tile0 = 0; tile0 < tiles; tile0 += tile_chunk) {
            for (uint32_t s0 = 0; s0 < n_k; s0 += sample_chunk) {
                g.tile0 = tile0;
                g.n_tiles = std::min(tile_chunk, tiles - tile0);
                g.n_samples = std::min(sample_chunk, n_k - s0);
                g.seed0 = frame0 + k * 64u + s0;
                g.first = s0 == 0 ? 1u : 0u;
                if (phases) if (int rc = phases->mark(stream)) return rc;
                HIP_TRY(launch_light_rays(g, stream));
                // (from here on the slot is this stream's: the rays launch below finds it by its stream)
                slot->last_stream = stream;
                slot->last_use = ++s->launches;
                HIP_TRY(hipEventRecord(slot->done.get(), stream));
                slot->used = true;
                if (phases) if (int rc = phases->mark(stream)) return rc;
                TraceParams p;
                std::memset(&p, 0, sizeof(p));
                p.rays = g.rays;
                p.out = reinterpret_cast<trx_hit *>(slot->ao_flags.get());
                p.any_hit = 1u;
                p.ray_mask = ray_mask; // (0: the unmasked launch; enqueue_locked hands a masked one the scene's table)
                p.n_items = g.n_tiles * g.n_samples * 64u;
                SlotCounters *ctr = nullptr;
                if (int rc = enqueue_locked(s, p, kModeRays, sem, false, stream, &ctr)) return rc;
                if (ctr != slot->ctr.get()) return fail(TRX_ERR_INVALID, "internal: the rays launch left the pass's launch slot");
                if (phases) if (int rc = phases->mark(stream)) return rc;
                HIP_TRY(launch_light_reduce(g, stream));
                HIP_TRY(hipEventRecord(slot->done.get(), stream));
                if (phases) if (int rc = phases->mark(stream)) return rc;
            }
        }
    }
    return TRX_OK;
}

// ---- the emitter light pass at primary hits (include/trx.h, "emitters", rules E1-E5) --------------------------------------------

void emitter_scene(EmitterParams &g, const trx_scene *s, const trx_hit *d_primary, const uint32_t *d_primary_inst) {
    g.tris = s->tris.get();
    g.inst_xform = s->tlas ? s->inst_xform.get() : nullptr;
    g.primary = d_primary;
    g.primary_inst = g.inst_xform ? d_primary_inst : nullptr;
    g.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull); // (kernels.h, surface_record)
    g.n_inst = s->n_inst;
    g.emitters = s->emitters.get();
    g.cdf = s->emitter_cdf.get();
    g.n_emitters = s->n_emitters;
}

// light_visibility_impl's sibling with the emitter table for the light: its chunk loops and slot bookkeeping, k_emitter_rays
// and k_emitter_gather_rgb around the rays launch; the running sums of a tile chunk sit in the slot's em_acc between its
// sample chunks, and the gather of the last one writes the planes (base read first: it may be the output).
int emitter_light_impl(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                       uint32_t frame0, uint32_t n_samples, float shadow_eps, float emitter_eps, const trx_hit *d_primary,
                       const uint32_t *d_primary_inst, const float *d_base, float *d_out, hipStream_t stream) {
    if (!s || !d_primary || !d_out) return fail(TRX_ERR_INVALID, "null argument");
    if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (ray_mask > 0xffu) return fail(TRX_ERR_INVALID, "ray_mask 0x%x outside 0..255", ray_mask);
    if (int rc = check_eps(shadow_eps)) return rc;
    if (int rc = check_emitter_eps(emitter_eps)) return rc;
    AoRaysParams geom;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(geom, view, w, h, shard, tiles)) return rc;
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    const uint64_t records = geom.geom.compact ? (uint64_t)tiles * 64u : (uint64_t)w * h;
    if (records > 0x7fffffffull) return fail(TRX_ERR_INVALID, "image %ux%u", w, h);
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    if (int rc = need_emitters(s)) return rc;
    if (tiles == 0) return TRX_OK;
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    EmitterParams g;
    std::memset(&g, 0, sizeof(g));
    g.geom = geom.geom;
    g.view = geom.view;
    emitter_scene(g, s, d_primary, d_primary_inst);
    g.materials = s->materials.get();
    g.scratch = 1u;
    g.shadow_eps = shadow_eps;
    g.emitter_eps = emitter_eps;
    g.n_total = n_samples;
    g.base = d_base;
    g.value = d_out;
    g.plane = (uint32_t)records;
    // chunks: as many tiles as the scratch holds, and for them as many samples as it holds (a unit of its own: kEmitterUnitBytes)
    const uint64_t units = std::min<uint64_t>(std::max<uint64_t>(g_ao_scratch_cap.load(std::memory_order_relaxed) / kEmitterUnitBytes, 1), 1ull << 24);
    const uint32_t tile_chunk = (uint32_t)std::min<uint64_t>(tiles, units);
    const uint32_t sample_chunk = (uint32_t)std::min<uint64_t>(n_samples, std::max<uint64_t>(units / tile_chunk, 1));
    const uint64_t rays = (uint64_t)tile_chunk * sample_chunk * 64, pixels = (uint64_t)tile_chunk * 64 * 3;
    if (slot->ao_rays.count() < rays || slot->em_wgeo.count() < rays || slot->em_pick.count() < rays || slot->em_acc.count() < pixels) {
        // (the slot's previous kernel may still be walking the old scratch)
        if (slot->used) HIP_TRY(hipEventSynchronize(slot->done.get()));
        if (slot->ao_rays.count() < rays) {
            slot->ao_flags.reset();
            HIP_TRY(slot->ao_rays.alloc(rays));
            HIP_TRY(slot->ao_flags.alloc(rays));
        }
        HIP_TRY(slot->em_wgeo.grow(rays));
        HIP_TRY(slot->em_pick.grow(rays));
        HIP_TRY(slot->em_acc.grow(pixels));
    }
    g.rays = slot->ao_rays.get();
    g.flags = slot->ao_flags.get();
    g.wgeo = slot->em_wgeo.get();
    g.pick = slot->em_pick.get();
    g.acc = slot->em_acc.get();
    for (uint32_t tile0 = 0; tile0 < tiles; tile0 += tile_chunk) {
        for (uint32_t s0 = 0; s0 < n_samples; s0 += sample_chunk) {
            g.tile0 = tile0;
            g.n_tiles = std::min(tile_chunk, tiles - tile0);
            g.n_samples = std::min(sample_chunk, n_samples - s0);
            g.seed0 = frame0 + 2048u + s0;
            g.first = s0 == 0 ? 1u : 0u;
            g.last = s0 + g.n_samples == n_samples ? 1u : 0u;
            HIP_TRY(launch_emitter_rays(g, stream));
            // (from here on the slot is this stream's: the rays launch below finds it by its stream)
            slot->last_stream = stream;
            slot->last_use = ++s->launches;
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            slot->used = true;
            TraceParams p;
            std::memset(&p, 0, sizeof(p));
            p.rays = g.rays;
            p.out = reinterpret_cast<trx_hit *>(slot->ao_flags.get());
            p.any_hit = 1u;
            p.ray_mask = ray_mask; // (0: the unmasked launch; enqueue_locked hands a masked one the scene's table)
            p.n_items = g.n_tiles * g.n_samples * 64u;
            SlotCounters *ctr = nullptr;
            if (int rc = enqueue_locked(s, p, kModeRays, sem, false, stream, &ctr)) return rc;
            if (ctr != slot->ctr.get()) return fail(TRX_ERR_INVALID, "internal: the rays launch left the pass's launch slot");
            HIP_TRY(launch_emitter_gather(g, stream));
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
        }
    }
    return TRX_OK;
}

// ---- one-bounce indirect light (include/trx.h, "indirect light") ----------------------------------------------------------------

// hipEvents around the launches of the indirect pass (trx_debug_indirect_phases): every mark but a chunk's first ends an
// interval that belongs to one of the six phases
enum BouncePhase : int { kPhStart = -1, kPhBounceRays = 0, kPhBounceWalk, kPhAttr, kPhShadowRays, kPhShadowWalk, kPhWeightGather, kPhCount };
struct BouncePhases {
    std::vector<Event> ev;
    std::vector<int> ends;
    int mark(hipStream_t stream, int phase) {
        ev.emplace_back();
        ends.push_back(phase);
        HIP_TRY(ev.back().create());
        HIP_TRY(hipEventRecord(ev.back().get(), stream));
        return TRX_OK;
    }
};

// the image geometry of a call that regenerates no primary ray: no view is needed (ao_geometry copies one)
int bounce_geometry(TileGeom &geom, uint32_t w, uint32_t h, trx_shard shard, uint32_t &tiles) {
    const trx_view none{};
    AoRaysParams g;
    if (int rc = ao_geometry(g, &none, w, h, shard, tiles)) return rc;
    geom = g.geom;
    return TRX_OK;
}

// light_visibility_impl's sibling for one diffuse bounce.  Per chunk of (tiles, samples), [tile][sample][64] like the AO
// pass's scratch: k_ao_rays writes the bounce rays (tmax = FLT_MAX), the closest-hit rays launch walks them (unmasked, with
// instance ids), k_hit_attr in rays mode gives every hit its normal; then light after light k_bounce_light_rays, the any-hit
// rays launch with p.ray_mask, k_bounce_weight; k_bounce_gather adds the chunk's sums to the tiles' running sums, and after a
// tile chunk's last samples k_bounce_finish writes the values.  Sample chunks ascend inside a tile chunk, lights ascend inside
// a sample chunk: every float sum is formed in the header's order whatever the cap.
//   colour (trx_trace_indirect_rgb_dev / _rgb_sparse_dev, rule 5c): the same launches up to the weights; the gather and the
// finish are k_bounce_gather_rgb and k_bounce_finish_rgb (BounceParams::materials), the running sums three per tile pixel,
// d_value three planes; albedo and d_base are not looked at.  The tables are read under s->mu, where
// trx_scene_set_materials swaps them, and every launch of the pass is recorded on the slot before the lock is released.
//   emitters (trx_trace_indirect_rgb_emitters_dev / _sparse_dev, rule 5e; emitter_eps set): the colour mode with one more step
// per chunk after the lights - k_bounce_emitter_rays, the any-hit rays launch with p.ray_mask - and
// k_bounce_emitter_gather for the gather; wgeo and j of every ray sit in the slot's em_wgeo / em_pick, 8 bytes per ray
// that this mode alone adds to its chunking unit; n_lights may be 0.  The other modes' launches and accounting are untouched.
int indirect_impl(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                  const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float bounce_eps, float shadow_eps,
                  float albedo, const trx_hit *d_primary, const uint32_t *d_primary_inst, const float *d_base, float *d_value,
                  hipStream_t stream, BouncePhases *phases, const SparseGrid *sparse = nullptr, bool colour = false,
                  const float *emitter_eps = nullptr, bool textured = false) {
    if (!s || !d_primary || !d_value) return fail(TRX_ERR_INVALID, "null argument");
    if (colour) { // (a table once set is only ever replaced: what holds here holds under the pass's lock below)
        std::lock_guard<std::mutex> lock(s->mu);
        if (!s->materials) return fail(TRX_ERR_INVALID, "the scene has no materials (trx_scene_set_materials)");
        if (emitter_eps) if (int rc = need_emitters(s)) return rc; // (asked again under the pass's lock: a table can go stale)
    }
    if (emitter_eps) if (int rc = check_emitter_eps(*emitter_eps)) return rc;
    if (sparse) if (int rc = check_sparse(sparse->stride, sparse->phase)) return rc;
    if (emitter_eps && n_lights == 0) { // (the emitter mode alone runs without a light: what check_lights asks of the samples)
        if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
            return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    } else if (int rc = check_lights(lights, n_lights, n_samples)) return rc;
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (ray_mask > 0xffu) return fail(TRX_ERR_INVALID, "ray_mask 0x%x outside 0..255", ray_mask);
    if (!(bounce_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "bounce_eps %g: must be >= 0", (double)bounce_eps);
    if (int rc = check_eps(shadow_eps)) return rc;
    if (!std::isfinite(albedo)) return fail(TRX_ERR_INVALID, "bounce_albedo %g is not finite", (double)albedo);
    AoRaysParams g;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(g, view, w, h, shard, tiles)) return rc;
    if (sparse) {
        // (visibility_impl's statement: the full image's geometry stays in g.geom and g.view, the tiles are the low grid's)
        AoRaysParams lo;
        const uint32_t st = sparse->stride;
        if (int rc = ao_geometry(lo, view, (w + st - 1) / st, (h + st - 1) / st, shard, tiles)) return rc;
        g.lo = lo.geom;
        g.stride = st;
        g.px0 = sparse->phase % st;
        g.py0 = sparse->phase / st;
    }
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    // (colour: floats per plane of d_value - the light visibility pass's plane rule, the low grid's cells in the sparse form)
    const uint64_t plane = sparse ? (uint64_t)g.lo.width * g.lo.height : g.geom.compact ? (uint64_t)tiles * 64u : (uint64_t)w * h;
    if (colour && plane > 0x7fffffffull) return fail(TRX_ERR_INVALID, "image %ux%u", w, h);
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (emitter_eps) if (int rc = need_emitters(s)) return rc;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    // chunks: as many tiles as the scratch holds, and for them as many samples as it holds (a unit of its own: kBounceUnitBytes,
    // in the emitter mode with the 8 bytes per ray of wgeo and j)
    const uint64_t unit_bytes = emitter_eps ? kBounceUnitBytes + 64u * 8u : kBounceUnitBytes;
    const uint64_t units = std::min<uint64_t>(std::max<uint64_t>(g_ao_scratch_cap.load(std::memory_order_relaxed) / unit_bytes, 1), 1ull << 24);
    const uint32_t tile_chunk = (uint32_t)std::min<uint64_t>(tiles, units);
    const uint32_t sample_chunk = (uint32_t)std::min<uint64_t>(n_samples, std::max<uint64_t>(units / tile_chunk, 1));
    const uint64_t rays = (uint64_t)tile_chunk * sample_chunk * 64, pixels = (uint64_t)tile_chunk * 64 * (colour ? 3 : 1);
    if (emitter_eps && (slot->em_wgeo.count() < rays || slot->em_pick.count() < rays)) {
        // (the slot's previous kernel may still be reading the old scratch)
        if (slot->used) HIP_TRY(hipEventSynchronize(slot->done.get()));
        HIP_TRY(slot->em_wgeo.grow(rays));
        HIP_TRY(slot->em_pick.grow(rays));
    }
    if (slot->ao_rays.count() < rays || slot->gi_rays.count() < rays || slot->gi_acc.count() < pixels) {
        // (the slot's previous kernel may still be walking the old scratch)
        if (slot->used) HIP_TRY(hipEventSynchronize(slot->done.get()));
        if (slot->ao_rays.count() < rays) {
            slot->ao_flags.reset();
            HIP_TRY(slot->ao_rays.alloc(rays));
            HIP_TRY(slot->ao_flags.alloc(rays));
        }
        if (slot->gi_rays.count() < rays) {
            // (the rays last: their count is what says that all five are there)
            slot->gi_rays.reset();
            HIP_TRY(slot->gi_hits.alloc(rays));
            HIP_TRY(slot->gi_inst.alloc(rays));
            HIP_TRY(slot->gi_attr.alloc(rays));
            HIP_TRY(slot->gi_sum.alloc(rays));
            HIP_TRY(slot->gi_rays.alloc(rays));
        }
        HIP_TRY(slot->gi_acc.grow(pixels));
    }
    const bool xf = s->tlas && s->inst_xform;
    // the bounce rays: the AO pass's rays with bounce_eps for ao_eps and no radius
    g.tris = s->tris.get();
    g.inst_xform = xf ? s->inst_xform.get() : nullptr;
    g.primary = d_primary;
    g.primary_inst = g.inst_xform ? d_primary_inst : nullptr;
    g.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull); // (kernels.h, surface_record)
    g.n_inst = s->n_inst;
    g.rays = slot->gi_rays.get();
    g.scratch = 1u;
    g.ao_eps = bounce_eps;
    g.tmax = FLT_MAX;
    HitAttrParams at;
    std::memset(&at, 0, sizeof(at));
    at.tris = s->tris.get();
    at.inst_xform = g.inst_xform;
    at.rays = slot->gi_rays.get();
    at.hits = slot->gi_hits.get();
    at.inst = xf ? slot->gi_inst.get() : nullptr;
    at.out = slot->gi_attr.get();
    at.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull);
    at.n_inst = s->n_inst;
    BounceParams b;
    std::memset(&b, 0, sizeof(b));
    b.bounce_rays = slot->gi_rays.get();
    b.bounce_hits = slot->gi_hits.get();
    b.bounce_attr = slot->gi_attr.get();
    b.rays = slot->ao_rays.get();
    b.flags = slot->ao_flags.get();
    b.sum = slot->gi_sum.get();
    b.acc = slot->gi_acc.get();
    b.primary = d_primary;
    b.n_tris = g.n_tris;
    b.base = d_base;
    b.value = d_value;
    b.scratch = 1u;
    b.n_total = n_samples;
    b.geom = g.geom;
    b.shadow_eps = shadow_eps;
    b.albedo = albedo;
    b.stride = g.stride; // (0: the dense kernels)
    b.px0 = g.px0;
    b.py0 = g.py0;
    b.lo = g.lo;
    if (colour) {
        b.materials = s->materials.get();
        b.tri_material = s->tri_material.get();
        b.plane = (uint32_t)plane;
    }
    if (emitter_eps) {
        b.emitters = s->emitters.get();
        b.cdf = s->emitter_cdf.get();
        b.n_emitters = s->n_emitters;
        b.wgeo = slot->em_wgeo.get();
        b.pick = slot->em_pick.get();
        b.has_lights = n_lights ? 1u : 0u;
        b.emitter_eps = *emitter_eps;
    }
    // textured (trx_trace_indirect_rgb_textured_dev): with both a texcoord table and a texture set on the scene the gather is
    // k_bounce_gather_tex; with either missing the pointers stay null and the pass is the colour mode's, kernel for kernel
    if (textured && colour && s->texcoords && s->material_texture) {
        b.tex.texcoords = s->texcoords.get();
        b.tex.descs = s->tex_descs.get();
        b.tex.texels = s->texels.get();
        b.tex.material_texture = s->material_texture.get();
        b.tex.srgb = s->tex_srgb.get();
    }
    // one rays launch on the pass's slot (the slot is this stream's once the first kernel of the chunk is recorded)
    auto walk = [&](TraceParams &p) -> int {
        SlotCounters *ctr = nullptr;
        if (int rc = enqueue_locked(s, p, kModeRays, sem, false, stream, &ctr)) return rc;
        if (ctr != slot->ctr.get()) return fail(TRX_ERR_INVALID, "internal: the rays launch left the pass's launch slot");
        return TRX_OK;
    };
    for (uint32_t tile0 = 0; tile0 < tiles; tile0 += tile_chunk) {
        for (uint32_t s0 = 0; s0 < n_samples; s0 += sample_chunk) {
            g.tile0 = b.tile0 = tile0;
            g.n_tiles = b.n_tiles = std::min(tile_chunk, tiles - tile0);
            g.n_samples = b.n_samples = std::min(sample_chunk, n_samples - s0);
            g.frame = frame0 + s0;
            const uint32_t n_rays = g.n_tiles * g.n_samples * 64u;
            if (phases) if (int rc = phases->mark(stream, kPhStart)) return rc;
            HIP_TRY(launch_ao_rays(g, stream));
            slot->last_stream = stream;
            slot->last_use = ++s->launches;
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            slot->used = true;
            if (phases) if (int rc = phases->mark(stream, kPhBounceRays)) return rc;
            {
                TraceParams p;
                std::memset(&p, 0, sizeof(p));
                p.rays = slot->gi_rays.get();
                p.out = slot->gi_hits.get();
                p.out_inst = slot->gi_inst.get();
                p.n_items = n_rays;
                if (int rc = walk(p)) return rc;
            }
            if (phases) if (int rc = phases->mark(stream, kPhBounceWalk)) return rc;
            at.n_items = n_rays;
            HIP_TRY(launch_hit_attr(at, kAttrRays, stream));
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            if (phases) if (int rc = phases->mark(stream, kPhAttr)) return rc;
            for (uint32_t k = 0; k < n_lights; k++) {
                b.light = lights[k];
                b.seed0 = frame0 + k * 64u + s0;
                b.first = k == 0 ? 1u : 0u;
                HIP_TRY(launch_bounce_light_rays(b, stream));
                HIP_TRY(hipEventRecord(slot->done.get(), stream));
                if (phases) if (int rc = phases->mark(stream, kPhShadowRays)) return rc;
                TraceParams p;
                std::memset(&p, 0, sizeof(p));
                p.rays = slot->ao_rays.get();
                p.out = reinterpret_cast<trx_hit *>(slot->ao_flags.get());
                p.any_hit = 1u;
                p.ray_mask = ray_mask; // (0: the unmasked launch; enqueue_locked hands a masked one the scene's table)
                p.n_items = n_rays;
                if (int rc = walk(p)) return rc;
                if (phases) if (int rc = phases->mark(stream, kPhShadowWalk)) return rc;
                HIP_TRY(launch_bounce_weight(b, stream));
                HIP_TRY(hipEventRecord(slot->done.get(), stream));
                if (phases) if (int rc = phases->mark(stream, kPhWeightGather)) return rc;
            }
            if (emitter_eps) {
                // rule 5e's step: the shadow rays from the bounce hits toward the emitters their noise selects, walked like a light's
                b.seed0 = frame0 + 8192u + s0;
                HIP_TRY(launch_bounce_emitter_rays(b, stream));
                HIP_TRY(hipEventRecord(slot->done.get(), stream));
                TraceParams p;
                std::memset(&p, 0, sizeof(p));
                p.rays = slot->ao_rays.get();
                p.out = reinterpret_cast<trx_hit *>(slot->ao_flags.get());
                p.any_hit = 1u;
                p.ray_mask = ray_mask;
                p.n_items = n_rays;
                if (int rc = walk(p)) return rc;
            }
            b.first = s0 == 0 ? 1u : 0u;
            HIP_TRY(launch_bounce_gather(b, stream));
            if (s0 + g.n_samples == n_samples) HIP_TRY(launch_bounce_finish(b, stream));
            HIP_TRY(hipEventRecord(slot->done.get(), stream));
            if (phases) if (int rc = phases->mark(stream, kPhWeightGather)) return rc;
        }
    }
    return TRX_OK;
}

} // namespace

// what every light entry point refuses of its lights and sample count (api_image.cpp's trx_render_image_lit asks too)
int trxapi::check_lights(const trx_light *lights, uint32_t n_lights, uint32_t n_samples) {
    if (n_lights == 0 || n_lights > TRX_MAX_LIGHTS) return fail(TRX_ERR_INVALID, "n_lights %u outside 1..%d", n_lights, TRX_MAX_LIGHTS);
    if (!lights) return fail(TRX_ERR_INVALID, "null lights");
    if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    for (uint32_t k = 0; k < n_lights; k++) {
        const trx_light &l = lights[k];
        if (l.kind > TRX_LIGHT_RECT) return fail(TRX_ERR_INVALID, "light %u: unknown kind %u", k, l.kind);
        for (uint32_t pad : l._pad)
            if (pad != 0u) return fail(TRX_ERR_INVALID, "light %u: _pad must be 0", k);
        bool finite = std::isfinite(l.intensity);
        for (int i = 0; i < 3; i++) finite = finite && std::isfinite(l.position[i]) && std::isfinite(l.edge1[i]) && std::isfinite(l.edge2[i]);
        if (!finite) return fail(TRX_ERR_INVALID, "light %u: a field is not finite", k);
        if (l.kind == TRX_LIGHT_DIRECTIONAL && l.position[0] == 0.0f && l.position[1] == 0.0f && l.position[2] == 0.0f)
            return fail(TRX_ERR_INVALID, "light %u: a directional light of zero length", k);
    }
    return TRX_OK;
}

extern "C" {

int trx_ao_rays_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t frame, float ao_eps,
                    float ao_radius, const trx_hit *d_primary, const uint32_t *d_primary_inst, trx_ray *d_rays, void *stream) {
    if (!s || !d_primary || !d_rays) return fail(TRX_ERR_INVALID, "null argument");
    AoRaysParams g;
    uint32_t tiles = 0;
    float tmax = 0.f;
    if (int rc = radius_tmax(ao_radius, tmax)) return rc;
    if (int rc = ao_geometry(g, view, w, h, shard, tiles)) return rc;
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, (hipStream_t)stream, slot)) return rc;
    g.tris = s->tris.get();
    g.inst_xform = s->tlas ? s->inst_xform.get() : nullptr;
    g.primary = d_primary;
    g.primary_inst = g.inst_xform ? d_primary_inst : nullptr;
    g.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull); // (kernels.h, surface_record)
    g.n_inst = s->n_inst;
    g.rays = d_rays;
    g.n_tiles = tiles;
    g.n_samples = 1u;
    g.frame = frame;
    g.ao_eps = ao_eps;
    g.tmax = tmax;
    slot->last_stream = (hipStream_t)stream;
    slot->last_use = ++s->launches;
    HIP_TRY(launch_ao_rays(g, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(slot->done.get(), (hipStream_t)stream));
    slot->used = true;
    return TRX_OK;
}

int trx_trace_ao_visibility_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem,
                                uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius, const trx_hit *d_primary,
                                const uint32_t *d_primary_inst, uint8_t *d_unoccluded, void *stream) {
    return visibility_impl(s, view, w, h, shard, sem, frame0, n_samples, ao_eps, ao_radius, d_primary, d_primary_inst,
                           d_unoccluded, (hipStream_t)stream, nullptr);
}

int trx_trace_ao_visibility_sparse_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase,
                                       uint32_t sem, uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius,
                                       const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_unoccluded_lo, void *stream) {
    const SparseGrid grid{stride, phase};
    return visibility_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, frame0, n_samples, ao_eps, ao_radius, d_primary, d_primary_inst,
                           d_unoccluded_lo, (hipStream_t)stream, nullptr, &grid);
}

int trx_trace_ao_visibility(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t frame0,
                            uint32_t n_samples, float ao_eps, float ao_radius, uint8_t *out_unoccluded, float *out_ms) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    float tmax = 0.f;
    if (int rc = radius_tmax(ao_radius, tmax)) return rc; // (before the primary pass)
    const uint64_t n = (uint64_t)w * h;
    const trx_shard whole{0, 1, 0, 0};
    // (the counts go where the AO records of trx_trace_primary_ao go: n bytes of the second record buffer)
    auto d_counts = [&] { return reinterpret_cast<uint8_t *>(s->scratch_b.get()); };
    return host_call(
        s, n, nullptr, 0, 0, out_ms,
        [&] {
            int rc = trx_trace_primary_inst_dev(s, view, w, h, whole, sem, s->scratch_a.get(), s->scratch_ia.get(), nullptr);
            if (rc) return rc;
            return trx_trace_ao_visibility_dev(s, view, w, h, whole, sem, frame0, n_samples, ao_eps, ao_radius,
                                               s->scratch_a.get(), s->scratch_ia.get(), d_counts(), nullptr);
        },
        [&]() -> int {
            if (out_unoccluded) HIP_TRY(hipMemcpy(out_unoccluded, d_counts(), n, hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

// ---- direct light -----------------------------------------------------------------------------------------------------------

int trx_light_rays_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, const trx_light *light,
                       uint32_t light_index, uint32_t frame0, uint32_t sample, float shadow_eps, const trx_hit *d_primary,
                       const uint32_t *d_primary_inst, trx_ray *d_rays, void *stream) {
    if (!s || !d_primary || !d_rays) return fail(TRX_ERR_INVALID, "null argument");
    if (int rc = check_lights(light, 1, 1)) return rc;
    if (light_index >= TRX_MAX_LIGHTS) return fail(TRX_ERR_INVALID, "light_index %u outside 0..%d", light_index, TRX_MAX_LIGHTS - 1);
    if (sample >= TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "sample %u outside 0..%d", sample, TRX_MAX_AO_SAMPLES - 1);
    if (int rc = check_eps(shadow_eps)) return rc;
    AoRaysParams geom;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(geom, view, w, h, shard, tiles)) return rc;
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, (hipStream_t)stream, slot)) return rc;
    LightRaysParams g;
    std::memset(&g, 0, sizeof(g));
    g.geom = geom.geom;
    g.view = geom.view;
    light_scene(g, s, d_primary, d_primary_inst);
    g.rays = d_rays;
    g.n_tiles = tiles;
    g.n_samples = 1u;
    g.seed0 = frame0 + light_index * 64u + sample;
    g.shadow_eps = shadow_eps;
    g.light = *light;
    slot->last_stream = (hipStream_t)stream;
    slot->last_use = ++s->launches;
    HIP_TRY(launch_light_rays(g, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(slot->done.get(), (hipStream_t)stream));
    slot->used = true;
    return TRX_OK;
}

int trx_trace_light_visibility_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem,
                                   uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                   float shadow_eps, const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_lit,
                                   void *stream) {
    return light_visibility_impl(s, view, w, h, shard, sem, ray_mask, lights, n_lights, frame0, n_samples, shadow_eps, d_primary,
                                 d_primary_inst, d_lit, (hipStream_t)stream, nullptr);
}

int trx_light_term_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, const trx_light *lights,
                       uint32_t n_lights, uint32_t n_samples, const trx_hit *d_primary, const trx_hit_attr *d_attr,
                       const uint8_t *d_lit, const trx_ao_term *d_term, float ambient, float *d_value, void *stream) {
    if (!s || !d_primary || !d_attr || !d_lit || !d_value) return fail(TRX_ERR_INVALID, "null argument");
    if (int rc = check_lights(lights, n_lights, n_samples)) return rc;
    if (!std::isfinite(ambient)) return fail(TRX_ERR_INVALID, "ambient %g is not finite", (double)ambient);
    AoRaysParams geom;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(geom, view, w, h, shard, tiles)) return rc;
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, (hipStream_t)stream, slot)) return rc;
    LightTermParams p;
    std::memset(&p, 0, sizeof(p));
    p.primary = d_primary;
    p.attr = d_attr;
    p.lit = d_lit;
    p.term = d_term;
    p.value = d_value;
    p.n_tiles = tiles;
    p.n_lights = n_lights;
    p.n_samples = n_samples;
    p.plane_stride = geom.geom.compact ? tiles * 64u : w * h;
    p.ambient = ambient;
    p.geom = geom.geom;
    p.view = geom.view;
    std::memcpy(p.lights, lights, n_lights * sizeof(trx_light));
    slot->last_stream = (hipStream_t)stream;
    slot->last_use = ++s->launches;
    HIP_TRY(launch_light_term(p, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(slot->done.get(), (hipStream_t)stream));
    slot->used = true;
    return TRX_OK;
}

// ---- one-bounce indirect light ------------------------------------------------------------------------------------------------

int trx_bounce_light_rays_dev(trx_scene *s, uint32_t w, uint32_t h, trx_shard shard, const trx_light *light, uint32_t light_index,
                              uint32_t frame0, uint32_t sample, float shadow_eps, const trx_ray *d_bounce_rays,
                              const trx_hit *d_bounce_hits, const trx_hit_attr *d_bounce_attr, trx_ray *d_rays, void *stream) {
    if (!s || !d_bounce_rays || !d_bounce_hits || !d_bounce_attr || !d_rays) return fail(TRX_ERR_INVALID, "null argument");
    if (int rc = check_lights(light, 1, 1)) return rc;
    if (light_index >= TRX_MAX_LIGHTS) return fail(TRX_ERR_INVALID, "light_index %u outside 0..%d", light_index, TRX_MAX_LIGHTS - 1);
    if (sample >= TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "sample %u outside 0..%d", sample, TRX_MAX_AO_SAMPLES - 1);
    if (int rc = check_eps(shadow_eps)) return rc;
    BounceParams b;
    std::memset(&b, 0, sizeof(b));
    uint32_t tiles = 0;
    if (int rc = bounce_geometry(b.geom, w, h, shard, tiles)) return rc;
    if (tiles == 0) return TRX_OK;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, (hipStream_t)stream, slot)) return rc;
    b.bounce_rays = d_bounce_rays;
    b.bounce_hits = d_bounce_hits;
    b.bounce_attr = d_bounce_attr;
    b.rays = d_rays;
    b.n_tiles = tiles;
    b.n_samples = 1u;
    b.seed0 = frame0 + light_index * 64u + sample;
    b.shadow_eps = shadow_eps;
    b.light = *light;
    slot->last_stream = (hipStream_t)stream;
    slot->last_use = ++s->launches;
    HIP_TRY(launch_bounce_light_rays(b, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(slot->done.get(), (hipStream_t)stream));
    slot->used = true;
    return TRX_OK;
}

int trx_trace_indirect_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                           const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float bounce_eps,
                           float shadow_eps, float bounce_albedo, const trx_hit *d_primary, const uint32_t *d_primary_inst,
                           const float *d_base, float *d_value, void *stream) {
    return indirect_impl(s, view, w, h, shard, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps, bounce_albedo,
                         d_primary, d_primary_inst, d_base, d_value, (hipStream_t)stream, nullptr);
}

int trx_trace_indirect_sparse_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase, uint32_t sem,
                                  uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                  float bounce_eps, float shadow_eps, float bounce_albedo, const trx_hit *d_primary,
                                  const uint32_t *d_primary_inst, float *d_value_lo, void *stream) {
    const SparseGrid grid{stride, phase};
    return indirect_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps,
                         bounce_albedo, d_primary, d_primary_inst, nullptr, d_value_lo, (hipStream_t)stream, nullptr, &grid);
}

// ---- the RGB indirect term (include/trx.h, "materials", rule 5c) -----------------------------------------------------------------

int trx_trace_indirect_rgb_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                               const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float bounce_eps,
                               float shadow_eps, const trx_hit *d_primary, const uint32_t *d_primary_inst, float *d_value_rgb, void *stream) {
    return indirect_impl(s, view, w, h, shard, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps, 1.0f, d_primary,
                         d_primary_inst, nullptr, d_value_rgb, (hipStream_t)stream, nullptr, nullptr, true);
}

int trx_trace_indirect_rgb_sparse_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase,
                                      uint32_t sem, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                      uint32_t n_samples, float bounce_eps, float shadow_eps, const trx_hit *d_primary,
                                      const uint32_t *d_primary_inst, float *d_value_rgb_lo, void *stream) {
    const SparseGrid grid{stride, phase};
    return indirect_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps,
                         1.0f, d_primary, d_primary_inst, nullptr, d_value_rgb_lo, (hipStream_t)stream, nullptr, &grid, true);
}

// ---- emitters (include/trx.h, "emitters") ---------------------------------------------------------------------------------------

int trx_emitter_rays_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t frame0, uint32_t sample,
                         float shadow_eps, float emitter_eps, const trx_hit *d_primary, const uint32_t *d_primary_inst, trx_ray *d_rays,
                         void *stream) {
    if (!s || !d_primary || !d_rays) return fail(TRX_ERR_INVALID, "null argument");
    if (sample >= TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "sample %u outside 0..%d", sample, TRX_MAX_AO_SAMPLES - 1);
    if (int rc = check_eps(shadow_eps)) return rc;
    if (int rc = check_emitter_eps(emitter_eps)) return rc;
    AoRaysParams geom;
    uint32_t tiles = 0;
    if (int rc = ao_geometry(geom, view, w, h, shard, tiles)) return rc;
    if (int rc = need_inst(s, d_primary_inst)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    if (int rc = need_emitters(s)) return rc;
    if (tiles == 0) return TRX_OK;
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, (hipStream_t)stream, slot)) return rc;
    EmitterParams g;
    std::memset(&g, 0, sizeof(g));
    g.geom = geom.geom;
    g.view = geom.view;
    emitter_scene(g, s, d_primary, d_primary_inst);
    g.rays = d_rays;
    g.n_tiles = tiles;
    g.n_samples = 1u;
    g.seed0 = frame0 + 2048u + sample;
    g.shadow_eps = shadow_eps;
    g.emitter_eps = emitter_eps;
    slot->last_stream = (hipStream_t)stream;
    slot->last_use = ++s->launches;
    HIP_TRY(launch_emitter_rays(g, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(slot->done.get(), (hipStream_t)stream));
    slot->used = true;
    return TRX_OK;
}

int trx_trace_emitter_light_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem, uint32_t ray_mask,
                                uint32_t frame0, uint32_t n_samples, float shadow_eps, float emitter_eps, const trx_hit *d_primary,
                                const uint32_t *d_primary_inst, const float *d_base_rgb, float *d_out_rgb, void *stream) {
    return emitter_light_impl(s, view, w, h, shard, sem, ray_mask, frame0, n_samples, shadow_eps, emitter_eps, d_primary, d_primary_inst,
                              d_base_rgb, d_out_rgb, (hipStream_t)stream);
}

int trx_trace_indirect_rgb_emitters_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t sem,
                                        uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples,
                                        float bounce_eps, float shadow_eps, float emitter_eps, const trx_hit *d_primary,
                                        const uint32_t *d_primary_inst, float *d_value_rgb, void *stream) {
    return indirect_impl(s, view, w, h, shard, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps, 1.0f, d_primary,
                         d_primary_inst, nullptr, d_value_rgb, (hipStream_t)stream, nullptr, nullptr, true, &emitter_eps);
}

int trx_trace_indirect_rgb_emitters_sparse_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase,
                                               uint32_t sem, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                                               uint32_t n_samples, float bounce_eps, float shadow_eps, float emitter_eps,
                                               const trx_hit *d_primary, const uint32_t *d_primary_inst, float *d_value_rgb_lo,
                                               void *stream) {
    const SparseGrid grid{stride, phase};
    return indirect_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps,
                         1.0f, d_primary, d_primary_inst, nullptr, d_value_rgb_lo, (hipStream_t)stream, nullptr, &grid, true, &emitter_eps);
}

// ---- the textured RGB indirect term (include/trx.h, "texture coordinates and albedo textures") -----------------------------------------

// One entry point for the four RGB modes: stride 1 is the dense pass over `shard`, stride 2.. the sparse pass over the whole
// image; use_emitters selects rule 5e.  Everything but the gather is the existing passes' (indirect_impl's `textured`).
int trx_trace_indirect_rgb_textured_dev(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard, uint32_t stride,
                                        uint32_t phase, uint32_t sem, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                                        uint32_t frame0, uint32_t n_samples, float bounce_eps, float shadow_eps, uint32_t use_emitters,
                                        float emitter_eps, const trx_hit *d_primary, const uint32_t *d_primary_inst, float *d_value_rgb,
                                        void *stream) {
    if (use_emitters > 1u) return fail(TRX_ERR_INVALID, "use_emitters %u: must be 0 or 1", use_emitters);
    if (int rc = check_sparse(stride, phase)) return rc;
    const float *eps = use_emitters ? &emitter_eps : nullptr;
    if (stride == 1u)
        return indirect_impl(s, view, w, h, shard, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps, 1.0f, d_primary,
                             d_primary_inst, nullptr, d_value_rgb, (hipStream_t)stream, nullptr, nullptr, true, eps, true);
    if (shard.index != 0u || shard.count != 1u || shard.layout != TRX_LAYOUT_IMAGE)
        return fail(TRX_ERR_INVALID, "stride %u: the sparse pass takes the whole image (shard {0, 1, TRX_LAYOUT_IMAGE})", stride);
    const SparseGrid grid{stride, phase};
    return indirect_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps, shadow_eps,
                         1.0f, d_primary, d_primary_inst, nullptr, d_value_rgb, (hipStream_t)stream, nullptr, &grid, true, eps, true);
}

// ---- development surface (include/trx_dev.h) ---------------------------------------------------------------------------

uint64_t trx_debug_ao_scratch_cap(uint64_t bytes) {
    return g_ao_scratch_cap.exchange(bytes ? bytes : kAoScratchCapDefault, std::memory_order_relaxed);
}

int trx_debug_ao_visibility_phases(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t frame0,
                                   uint32_t n_samples, float ao_eps, float ao_radius, const trx_hit *d_primary,
                                   const uint32_t *d_primary_inst, uint8_t *d_unoccluded, float out_ms[3]) {
    if (!s || !out_ms) return fail(TRX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    Phases ph;
    if (int rc = visibility_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, frame0, n_samples, ao_eps, ao_radius, d_primary,
                                 d_primary_inst, d_unoccluded, nullptr, &ph))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    out_ms[0] = out_ms[1] = out_ms[2] = 0.f;
    for (size_t c = 0; c + 3 < ph.ev.size(); c += 4)
        for (int k = 0; k < 3; k++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ph.ev[c + k].get(), ph.ev[c + k + 1].get()));
            out_ms[k] += ms;
        }
    return trx_scene_check(s, nullptr);
}

int trx_debug_light_visibility_phases(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                      const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float shadow_eps,
                                      const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_lit, float out_ms[3]) {
    if (!s || !out_ms) return fail(TRX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    Phases ph;
    if (int rc = light_visibility_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples,
                                       shadow_eps, d_primary, d_primary_inst, d_lit, nullptr, &ph))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    out_ms[0] = out_ms[1] = out_ms[2] = 0.f;
    for (size_t c = 0; c + 3 < ph.ev.size(); c += 4)
        for (int k = 0; k < 3; k++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ph.ev[c + k].get(), ph.ev[c + k + 1].get()));
            out_ms[k] += ms;
        }
    return trx_scene_check(s, nullptr);
}

int trx_debug_indirect_phases(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                              const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t n_samples, float bounce_eps,
                              float shadow_eps, float bounce_albedo, const trx_hit *d_primary, const uint32_t *d_primary_inst,
                              const float *d_base, float *d_value, float out_ms[6]) {
    if (!s || !out_ms) return fail(TRX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    BouncePhases ph;
    if (int rc = indirect_impl(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, ray_mask, lights, n_lights, frame0, n_samples, bounce_eps,
                               shadow_eps, bounce_albedo, d_primary, d_primary_inst, d_base, d_value, nullptr, &ph))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (int k = 0; k < kPhCount; k++) out_ms[k] = 0.f;
    for (size_t i = 1; i < ph.ev.size(); i++) {
        if (ph.ends[i] < 0) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ph.ev[i - 1].get(), ph.ev[i].get()));
        out_ms[ph.ends[i]] += ms;
    }
    return trx_scene_check(s, nullptr);
}

} // extern "C"
