// api_image.cpp - the frame's image (include/trx.h, trx_ao_filter_dev / trx_ao_upsample_dev / trx_shade_*_dev /
// trx_render_image*, trx_render_image_lit among them): the edge-aware filter over the AO visibility pass's counts, the edge-aware upsample of the sparse
// pass's counts and the shading to RGBA8 (k_ao_filter, k_ao_upsample, k_shade, image.hip), the a-trous filter over float
// planes (trx_value_filter_dev / trx_render_image_gi_filtered, k_atrous), the edge-aware upsample of a low-grid float plane (trx_value_upsample_dev / trx_render_image_gi_sparse, k_plane_upsample), and the table of
// code thresholds the shade searches instead of evaluating pow; the PROFILE_RT heat map of a counting pass's per-ray counts
// (trx_shade_heat_dev / trx_render_heat_image, k_heat).  Image passes after the walk: none reads scene data, but
// each takes a launch slot of the scene like the attribute pass, so trx_scene_refit waits for them.
#include "api_internal.h"

#include <cfloat>
#include <limits>

namespace {

// The reference's colour code on this host (src/rt_cpu/rt_cpu.rs:102-112, cli.cpp save_png), for col in [0, 1].
uint32_t host_code(float col) { return (uint32_t)(uint8_t)(uint32_t)(::powf(col, 2.2f) * 255.0f); }

// thr[k], k = 1..255: the smallest binary32 in [0, 1] whose host code is >= k, by bisection over the bit pattern (the
// patterns of the non-negative floats are ordered like their values); thr[0] = 0.
const float *code_table() {
    static float thr[256];
    static std::once_flag once;
    std::call_once(once, [] {
        const float one = 1.0f;
        uint32_t one_bits;
        std::memcpy(&one_bits, &one, 4);
        thr[0] = 0.0f;
        for (uint32_t k = 1; k < 256; k++) {
            if (host_code(one) < k) { // (no colour reaches the code: never the case with a powf that returns 1 for 1)
                thr[k] = std::numeric_limits<float>::infinity();
                continue;
            }
            uint32_t lo = 0u, hi = one_bits; // code(lo) < k <= code(hi)
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                float x;
                std::memcpy(&x, &mid, 4);
                if (host_code(x) >= k) hi = mid;
                else lo = mid;
            }
            std::memcpy(&thr[k], &hi, 4);
        }
    });
    return thr;
}

int check_samples(uint32_t n_samples) {
    if (n_samples == 0 || n_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", n_samples, TRX_MAX_AO_SAMPLES);
    return TRX_OK;
}

int check_filter(uint32_t radius, float depth_tol, float normal_cos) {
    if (radius > TRX_MAX_AO_FILTER_RADIUS) return fail(TRX_ERR_INVALID, "filter radius %u beyond %d", radius, TRX_MAX_AO_FILTER_RADIUS);
    if (!(depth_tol >= 0.0f)) return fail(TRX_ERR_INVALID, "depth_tol %g: must be >= 0 (+inf allowed)", (double)depth_tol);
    if (normal_cos != normal_cos) return fail(TRX_ERR_INVALID, "normal_cos is NaN");
    return TRX_OK;
}

int check_sparse(uint32_t stride, uint32_t phase, uint32_t radius) {
    if (stride == 0 || stride > TRX_MAX_AO_STRIDE) return fail(TRX_ERR_INVALID, "stride %u outside 1..%d", stride, TRX_MAX_AO_STRIDE);
    if (phase >= stride * stride) return fail(TRX_ERR_INVALID, "phase %u outside 0..%u (stride %u)", phase, stride * stride - 1, stride);
    if (radius > TRX_MAX_AO_UPSAMPLE_RADIUS) return fail(TRX_ERR_INVALID, "upsample radius %u beyond %d", radius, TRX_MAX_AO_UPSAMPLE_RADIUS);
    return TRX_OK;
}

int check_image(uint32_t w, uint32_t h) {
    const uint64_t n = (uint64_t)w * h;
    if (n == 0 || n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "image %ux%u", w, h);
    return TRX_OK;
}

// A launch slot of the scene for `stream`, then `launch`, then the slot's event: what orders the pass with trx_scene_refit.
// (launch takes the slot: a pass with scratch of its own on the slot)
template <typename Launch>
int enqueue_image_slot(trx_scene *s, hipStream_t stream, bool need_table, Launch launch) {
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lock(s->mu);
    if (need_table && !s->image_thr) { // first shade on this scene: the code thresholds beside it on its device
        HIP_TRY(s->image_thr.alloc(256));
        if (hipError_t e = hipMemcpy(s->image_thr.get(), code_table(), 256 * sizeof(float), hipMemcpyHostToDevice); e != hipSuccess) {
            s->image_thr.reset();
            return fail(TRX_ERR_NO_DEVICE, "uploading the code table failed: %s", hipGetErrorString(e));
        }
    }
    Slot *slot = nullptr;
    if (int rc = acquire_slot(s, stream, slot)) return rc;
    slot->last_stream = stream;
    slot->last_use = ++s->launches;
    if (int rc = launch(*slot)) return rc;
    HIP_TRY(hipEventRecord(slot->done.get(), stream));
    slot->used = true;
    return TRX_OK;
}
template <typename Launch>
int enqueue_image(trx_scene *s, hipStream_t stream, bool need_table, Launch launch) {
    return enqueue_image_slot(s, stream, need_table, [&](Slot &) -> int { return launch(); });
}

int check_value_filter(uint32_t n_levels, float depth_tol, float normal_cos) {
    if (n_levels == 0 || n_levels > TRX_MAX_VALUE_FILTER_LEVELS)
        return fail(TRX_ERR_INVALID, "n_levels %u outside 1..%d", n_levels, TRX_MAX_VALUE_FILTER_LEVELS);
    if (!(depth_tol >= 0.0f)) return fail(TRX_ERR_INVALID, "depth_tol %g: must be >= 0 (+inf allowed)", (double)depth_tol);
    if (normal_cos != normal_cos) return fail(TRX_ERR_INVALID, "normal_cos is NaN");
    return TRX_OK;
}

// what trx_value_upsample_dev refuses of its numbers (trx_render_image_gi_sparse asks too)
int check_value_upsample(uint32_t stride, uint32_t phase, uint32_t radius, float depth_tol, float normal_cos) {
    if (int rc = check_sparse(stride, phase, 0u)) return rc;
    if (radius > TRX_MAX_VALUE_UPSAMPLE_RADIUS)
        return fail(TRX_ERR_INVALID, "upsample radius %u beyond %d", radius, TRX_MAX_VALUE_UPSAMPLE_RADIUS);
    if (!(depth_tol >= 0.0f)) return fail(TRX_ERR_INVALID, "depth_tol %g: must be >= 0 (+inf allowed)", (double)depth_tol);
    if (normal_cos != normal_cos) return fail(TRX_ERR_INVALID, "normal_cos is NaN");
    return TRX_OK;
}

// One k_shade pass over n records (launches of at most 2^30), on a launch slot.
int enqueue_shade(trx_scene *s, ShadeParams base, int mode, uint64_t n, hipStream_t stream) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (n == 0) return TRX_OK;
    if (!base.rgba || (mode == kShadeReference && (!base.primary || !base.ao)) || (mode == kShadeCounts && !base.counts) ||
        (mode == kShadeTerm && !base.term) || (mode == kShadeValue && !base.value))
        return fail(TRX_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(base.rgba) & 3u) return fail(TRX_ERR_INVALID, "d_rgba is not 4-byte aligned");
    return enqueue_image(s, stream, true, [&]() -> int {
        const uint64_t chunk = 1ull << 30;
        for (uint64_t off = 0; off < n; off += chunk) {
            ShadeParams p = base;
            p.thr = s->image_thr.get();
            if (p.primary) p.primary += off;
            if (p.ao) p.ao += off;
            if (p.counts) p.counts += off;
            if (p.term) p.term += off;
            if (p.value) p.value += off;
            p.rgba += off * 4;
            p.n_items = (uint32_t)std::min(chunk, n - off);
            HIP_TRY(launch_shade(p, mode, stream));
        }
        return TRX_OK;
    });
}

int check_heat(uint32_t which, float scale) {
    if (which > TRX_HEAT_TRIS) return fail(TRX_ERR_INVALID, "heat map of %u: TRX_HEAT_NODES or TRX_HEAT_TRIS", which);
    if (!(scale >= 0.0f) || scale > FLT_MAX) return fail(TRX_ERR_INVALID, "heat scale %g: must be finite and >= 0", (double)scale);
    return TRX_OK;
}

} // namespace

extern "C" {

int trx_image_code_table(float out[256]) {
    if (!out) return fail(TRX_ERR_INVALID, "null argument");
    std::memcpy(out, code_table(), 256 * sizeof(float));
    return TRX_OK;
}

int trx_ao_filter_dev(trx_scene *s, uint32_t w, uint32_t h, const trx_hit *d_primary, const trx_hit_attr *d_attr,
                      const uint8_t *d_unoccluded, uint32_t n_samples, uint32_t radius, float depth_tol, float normal_cos,
                      trx_ao_term *d_term, void *stream) {
    if (int rc = check_filter(radius, depth_tol, normal_cos)) return rc;
    if (int rc = check_samples(n_samples)) return rc;
    if (int rc = check_image(w, h)) return rc;
    if (!s || !d_primary || !d_unoccluded || !d_term) return fail(TRX_ERR_INVALID, "null argument");
    AoFilterParams p;
    std::memset(&p, 0, sizeof(p));
    p.primary = d_primary;
    p.attr = d_attr;
    p.counts = d_unoccluded;
    p.out = d_term;
    p.width = w;
    p.height = h;
    p.n_samples = n_samples;
    p.radius = radius;
    p.depth_tol = depth_tol;
    p.normal_cos = normal_cos;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        HIP_TRY(launch_ao_filter(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

int trx_ao_upsample_dev(trx_scene *s, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase, const trx_hit *d_primary,
                        const trx_hit_attr *d_attr, const uint8_t *d_unoccluded_lo, uint32_t n_samples, uint32_t radius, float depth_tol,
                        float normal_cos, trx_ao_term *d_term, void *stream) {
    if (int rc = check_sparse(stride, phase, radius)) return rc;
    if (int rc = check_filter(radius, depth_tol, normal_cos)) return rc;
    if (int rc = check_samples(n_samples)) return rc;
    if (int rc = check_image(w, h)) return rc;
    if (!s || !d_primary || !d_unoccluded_lo || !d_term) return fail(TRX_ERR_INVALID, "null argument");
    AoUpsampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.primary = d_primary;
    p.attr = d_attr;
    p.counts_lo = d_unoccluded_lo;
    p.out = d_term;
    p.width = w;
    p.height = h;
    p.lo_width = (w + stride - 1u) / stride;
    p.lo_height = (h + stride - 1u) / stride;
    p.stride = stride;
    p.px0 = phase % stride;
    p.py0 = phase / stride;
    p.n_samples = n_samples;
    p.radius = radius;
    p.depth_tol = depth_tol;
    p.normal_cos = normal_cos;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        HIP_TRY(launch_ao_upsample(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

int trx_shade_reference_dev(trx_scene *s, const trx_hit *d_primary, const trx_hit *d_ao, uint64_t n, uint8_t *d_rgba, void *stream) {
    ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.primary = d_primary;
    p.ao = d_ao;
    p.rgba = d_rgba;
    return enqueue_shade(s, p, kShadeReference, n, (hipStream_t)stream);
}

int trx_shade_ao_counts_dev(trx_scene *s, const uint8_t *d_unoccluded, uint32_t n_samples, uint64_t n, uint8_t *d_rgba, void *stream) {
    if (int rc = check_samples(n_samples)) return rc;
    ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.counts = d_unoccluded;
    p.n_samples = n_samples;
    p.rgba = d_rgba;
    return enqueue_shade(s, p, kShadeCounts, n, (hipStream_t)stream);
}

int trx_shade_ao_term_dev(trx_scene *s, const trx_ao_term *d_term, uint64_t n, uint8_t *d_rgba, void *stream) {
    ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.term = d_term;
    p.rgba = d_rgba;
    return enqueue_shade(s, p, kShadeTerm, n, (hipStream_t)stream);
}

int trx_shade_value_dev(trx_scene *s, const float *d_value, uint64_t n, uint8_t *d_rgba, void *stream) {
    ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.value = d_value;
    p.rgba = d_rgba;
    return enqueue_shade(s, p, kShadeValue, n, (hipStream_t)stream);
}

int trx_value_filter_dev(trx_scene *s, uint32_t w, uint32_t h, const trx_hit *d_primary, const trx_hit_attr *d_attr, const float *d_in,
                         const float *d_base, uint32_t n_levels, float depth_tol, float normal_cos, float *d_work, float *d_out,
                         void *stream) {
    if (int rc = check_value_filter(n_levels, depth_tol, normal_cos)) return rc;
    if (int rc = check_image(w, h)) return rc;
    if (!s || !d_primary || !d_in || !d_out) return fail(TRX_ERR_INVALID, "null argument");
    if (n_levels >= 2 && !d_work) return fail(TRX_ERR_INVALID, "null d_work with n_levels %u", n_levels);
    if (d_in == d_out) return fail(TRX_ERR_INVALID, "d_in is d_out: a level cannot run in place");
    if (d_work && (d_work == d_in || d_work == d_out || d_work == d_base))
        return fail(TRX_ERR_INVALID, "d_work is d_in, d_out or d_base");
    const uint64_t n = (uint64_t)w * h;
    // With d_base in d_out no level but the last may write d_out: the intermediate planes alternate between d_work and a
    // plane of the slot's.  Otherwise between d_work and d_out, so that the last level lands in d_out.
    const bool own_plane = d_base == d_out && n_levels >= 3;
    return enqueue_image_slot(s, (hipStream_t)stream, false, [&](Slot &slot) -> int {
        if (own_plane && slot.vf_plane.count() < n) {
            // (the slot's previous kernel may still be reading the old plane)
            if (slot.used) HIP_TRY(hipEventSynchronize(slot.done.get()));
            HIP_TRY(slot.vf_plane.grow(n));
        }
        const float *src = d_in;
        for (uint32_t j = 0; j < n_levels; j++) {
            const bool last = j + 1 == n_levels;
            float *dst = d_out;
            if (!last) dst = own_plane ? ((j & 1u) ? slot.vf_plane.get() : d_work) : (((n_levels - 1u - j) & 1u) ? d_work : d_out);
            AtrousParams p;
            std::memset(&p, 0, sizeof(p));
            p.primary = d_primary;
            p.attr = d_attr;
            p.in = src;
            p.base = last ? d_base : nullptr;
            p.out = dst;
            p.width = w;
            p.height = h;
            p.spacing = 1u << j;
            p.last = last ? 1u : 0u;
            p.depth_tol = depth_tol;
            p.normal_cos = normal_cos;
            HIP_TRY(launch_atrous(p, (hipStream_t)stream));
            src = dst;
        }
        return TRX_OK;
    });
}

int trx_value_upsample_dev(trx_scene *s, uint32_t w, uint32_t h, uint32_t stride, uint32_t phase, const trx_hit *d_primary,
                           const trx_hit_attr *d_attr, const float *d_in_lo, const float *d_base, uint32_t radius, float depth_tol,
                           float normal_cos, float *d_out, void *stream) {
    if (int rc = check_value_upsample(stride, phase, radius, depth_tol, normal_cos)) return rc;
    if (int rc = check_image(w, h)) return rc;
    if (!s || !d_primary || !d_in_lo || !d_out) return fail(TRX_ERR_INVALID, "null argument");
    if (d_in_lo == d_out) return fail(TRX_ERR_INVALID, "d_in_lo is d_out: the upsample cannot run in place");
    PlaneUpsampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.primary = d_primary;
    p.attr = d_attr;
    p.in_lo = d_in_lo;
    p.base = d_base;
    p.out = d_out;
    p.width = w;
    p.height = h;
    p.lo_width = (w + stride - 1u) / stride;
    p.lo_height = (h + stride - 1u) / stride;
    p.stride = stride;
    p.px0 = phase % stride;
    p.py0 = phase / stride;
    p.radius = radius;
    p.depth_tol = depth_tol;
    p.normal_cos = normal_cos;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        HIP_TRY(launch_plane_upsample(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

int trx_shade_heat_dev(trx_scene *s, const trx_ray_cost *d_cost, uint64_t n, uint32_t which, float scale, uint8_t *d_rgba,
                       void *stream) {
    if (int rc = check_heat(which, scale)) return rc;
    if (reinterpret_cast<uintptr_t>(d_rgba) & 3u) return fail(TRX_ERR_INVALID, "d_rgba is not 4-byte aligned");
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (n == 0) return TRX_OK;
    if (!d_cost || !d_rgba) return fail(TRX_ERR_INVALID, "null argument");
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        const uint64_t chunk = 1ull << 30;
        for (uint64_t off = 0; off < n; off += chunk) {
            HeatParams p;
            p.cost = d_cost + off;
            p.rgba = d_rgba + off * 4;
            p.n_items = (uint32_t)std::min(chunk, n - off);
            p.which = which;
            p.scale = scale;
            HIP_TRY(launch_heat(p, (hipStream_t)stream));
        }
        return TRX_OK;
    });
}

int trx_render_heat_image(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t which, float scale,
                          uint8_t *out_rgba, trx_stats *out_stats) {
    if (int rc = check_heat(which, scale)) return rc;
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (int rc = check_image(w, h)) return rc;
    if (!s || !view) return fail(TRX_ERR_INVALID, "null argument");
    const uint64_t n = (uint64_t)w * h;
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (trx_count_primary_per_ray takes it again: the image scratch is under it too)
    HIP_TRY(hipSetDevice(s->device));
    // the image scratch: the per-ray counts, then the image
    HIP_TRY(s->scratch_img.grow(n * 8));
    trx_ray_cost *const d_cost = reinterpret_cast<trx_ray_cost *>(s->scratch_img.get());
    uint8_t *const d_rgba = s->scratch_img.get() + n * 4;
    if (int rc = trx_count_primary_per_ray(s, view, w, h, trx_shard{0, 1, 0, 0}, sem, nullptr, d_cost, out_stats)) return rc;
    if (int rc = trx_shade_heat_dev(s, d_cost, n, which, scale, d_rgba, nullptr)) return rc;
    // (a blocking copy, or a wait: the shade has finished when this returns)
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, d_rgba, n * 4, hipMemcpyDeviceToHost));
    else HIP_TRY(hipStreamSynchronize(nullptr));
    return TRX_OK;
}

int trx_render_image(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t frame0, uint32_t n_samples,
                     float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol, float normal_cos, uint8_t *out_rgba,
                     float *out_ms) {
    if (n_samples > TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "n_samples %u outside 0..%d", n_samples, TRX_MAX_AO_SAMPLES);
    if (n_samples != 0) {
        if (!(ao_radius > 0.0f)) return fail(TRX_ERR_INVALID, "ao_radius %g: must be > 0 (+inf allowed)", (double)ao_radius);
        if (filter_radius != 0)
            if (int rc = check_filter(filter_radius, depth_tol, normal_cos)) return rc;
    }
    if (int rc = check_image(w, h)) return rc;
    if (!s || !view) return fail(TRX_ERR_INVALID, "null argument");
    const uint64_t n = (uint64_t)w * h;
    const trx_shard whole{0, 1, 0, 0};
    const bool filter = n_samples != 0 && filter_radius != 0;
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (host_call takes it again: the image scratch is under it too)
    HIP_TRY(hipSetDevice(s->device));
    // the image scratch: the filter's terms, then the image
    HIP_TRY(s->scratch_img.grow(n * 8));
    auto d_term = [&] { return reinterpret_cast<trx_ao_term *>(s->scratch_img.get()); };
    auto d_rgba = [&] { return s->scratch_img.get() + n * 4; };
    // (the counts go where trx_trace_ao_visibility puts them: n bytes of the second record buffer)
    auto d_counts = [&] { return reinterpret_cast<uint8_t *>(s->scratch_b.get()); };
    return host_call(
        s, n, nullptr, 0, filter ? n : 0, out_ms,
        [&] {
            int rc = trx_trace_primary_inst_dev(s, view, w, h, whole, sem, s->scratch_a.get(), s->scratch_ia.get(), nullptr);
            if (rc) return rc;
            if (n_samples == 0) {
                rc = trx_trace_ao_inst_dev(s, view, w, h, whole, sem, frame0, ao_eps, s->scratch_a.get(), s->scratch_ia.get(),
                                           s->scratch_b.get(), s->scratch_ib.get(), nullptr);
                if (rc) return rc;
                return trx_shade_reference_dev(s, s->scratch_a.get(), s->scratch_b.get(), n, d_rgba(), nullptr);
            }
            rc = trx_trace_ao_visibility_dev(s, view, w, h, whole, sem, frame0, n_samples, ao_eps, ao_radius, s->scratch_a.get(),
                                             s->scratch_ia.get(), d_counts(), nullptr);
            if (rc) return rc;
            if (!filter) return trx_shade_ao_counts_dev(s, d_counts(), n_samples, n, d_rgba(), nullptr);
            rc = trx_hit_attributes_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(), nullptr);
            if (rc) return rc;
            rc = trx_ao_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), d_counts(), n_samples, filter_radius, depth_tol,
                                   normal_cos, d_term(), nullptr);
            if (rc) return rc;
            return trx_shade_ao_term_dev(s, d_term(), n, d_rgba(), nullptr);
        },
        [&]() -> int {
            if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, d_rgba(), n * 4, hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

int trx_render_image_sparse(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t frame0,
                            uint32_t n_samples, float ao_eps, float ao_radius, uint32_t ao_stride, uint32_t ao_phase,
                            uint32_t upsample_radius, float depth_tol, float normal_cos, uint8_t *out_rgba, float *out_ms) {
    if (int rc = check_samples(n_samples)) return rc;
    if (!(ao_radius > 0.0f)) return fail(TRX_ERR_INVALID, "ao_radius %g: must be > 0 (+inf allowed)", (double)ao_radius);
    if (int rc = check_sparse(ao_stride, ao_phase, upsample_radius)) return rc;
    if (int rc = check_filter(upsample_radius, depth_tol, normal_cos)) return rc;
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (int rc = check_image(w, h)) return rc;
    if (!s || !view) return fail(TRX_ERR_INVALID, "null argument");
    const uint64_t n = (uint64_t)w * h;
    const trx_shard whole{0, 1, 0, 0};
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (host_call takes it again: the image scratch is under it too)
    HIP_TRY(hipSetDevice(s->device));
    // the image scratch: the upsampled terms, then the image
    HIP_TRY(s->scratch_img.grow(n * 8));
    auto d_term = [&] { return reinterpret_cast<trx_ao_term *>(s->scratch_img.get()); };
    auto d_rgba = [&] { return s->scratch_img.get() + n * 4; };
    // (the low grid's counts go where trx_trace_ao_visibility puts the dense ones: at most n bytes of the second record buffer)
    auto d_counts = [&] { return reinterpret_cast<uint8_t *>(s->scratch_b.get()); };
    return host_call(
        s, n, nullptr, 0, n, out_ms,
        [&] {
            int rc = trx_trace_primary_inst_dev(s, view, w, h, whole, sem, s->scratch_a.get(), s->scratch_ia.get(), nullptr);
            if (rc) return rc;
            rc = trx_hit_attributes_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(), nullptr);
            if (rc) return rc;
            rc = trx_trace_ao_visibility_sparse_dev(s, view, w, h, ao_stride, ao_phase, sem, frame0, n_samples, ao_eps, ao_radius,
                                                    s->scratch_a.get(), s->scratch_ia.get(), d_counts(), nullptr);
            if (rc) return rc;
            rc = trx_ao_upsample_dev(s, w, h, ao_stride, ao_phase, s->scratch_a.get(), s->scratch_attr.get(), d_counts(), n_samples,
                                     upsample_radius, depth_tol, normal_cos, d_term(), nullptr);
            if (rc) return rc;
            return trx_shade_ao_term_dev(s, d_term(), n, d_rgba(), nullptr);
        },
        [&]() -> int {
            if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, d_rgba(), n * 4, hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

// trx_render_image_lit (bounce_samples == 0), trx_render_image_gi (bounce_samples >= 1: the indirect pass between the light
// term and the shade, the term's values its base and its output) and trx_render_image_gi_filtered (filter_levels >= 1: the
// indirect pass without a base into a plane of its own, the value filter over that plane with the term's values its base and
// its output); trx_render_image_gi_sparse (bounce_stride >= 1: the sparse indirect pass into a low plane, then the upsample - with
// the term's values its base and its output, or with filter levels without a base into the plane the filter then reads).
// smooth (trx_render_image_lit_smooth): the shading-normal pass right after the attribute pass, in place - the light term, the
// filters and the upsample then read the shading attributes; the ray-generating passes take no attribute buffer.
// (the table is swapped under s->mu; a removal between this check and the pass makes the pass itself refuse)
static int need_vertex_normals(trx_scene *s) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->vertex_normals) return fail(TRX_ERR_INVALID, "the scene has no vertex normals (trx_scene_set_vertex_normals)");
    return TRX_OK;
}

static int render_lit(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                      const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                      float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                      float normal_cos, uint32_t bounce_samples, float bounce_eps, float bounce_albedo, uint32_t filter_levels,
                      float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase,
                      uint32_t upsample_radius, uint8_t *out_rgba, float *out_ms, bool smooth = false) {
    if (int rc = check_lights(lights, n_lights, light_samples)) return rc;
    if (ray_mask > 0xffu) return fail(TRX_ERR_INVALID, "ray_mask 0x%x outside 0..255", ray_mask);
    if (!(shadow_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "shadow_eps %g: must be >= 0", (double)shadow_eps);
    if (!std::isfinite(ambient)) return fail(TRX_ERR_INVALID, "ambient %g is not finite", (double)ambient);
    if (ao_samples > TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "ao_samples %u outside 0..%d", ao_samples, TRX_MAX_AO_SAMPLES);
    if (ao_samples != 0) {
        if (!(ao_radius > 0.0f)) return fail(TRX_ERR_INVALID, "ao_radius %g: must be > 0 (+inf allowed)", (double)ao_radius);
        if (int rc = check_filter(filter_radius, depth_tol, normal_cos)) return rc;
    }
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (int rc = check_image(w, h)) return rc;
    if (!s || !view) return fail(TRX_ERR_INVALID, "null argument");
    if (smooth)
        if (int rc = need_vertex_normals(s)) return rc;
    const uint64_t n = (uint64_t)w * h;
    const trx_shard whole{0, 1, 0, 0};
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (host_call takes it again: the image scratch is under it too)
    HIP_TRY(hipSetDevice(s->device));
    // the image scratch: the filter's terms, the image, the light term's values, with a value filter the indirect term and the
    // filter's work plane, with a sparse indirect pass its low plane (at most one plane), then the lights' planes
    const uint64_t planes = bounce_stride != 0 ? 6 : filter_levels != 0 ? 5 : 3;
    HIP_TRY(s->scratch_img.grow(n * 4 * planes + n * n_lights));
    auto d_term = [&] { return reinterpret_cast<trx_ao_term *>(s->scratch_img.get()); };
    auto d_rgba = [&] { return s->scratch_img.get() + n * 4; };
    auto d_value = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 8); };
    auto d_indirect = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 12); };
    auto d_work = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 16); };
    auto d_low = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 20); };
    auto d_lit = [&] { return s->scratch_img.get() + n * 4 * planes; };
    // (the AO counts go where trx_trace_ao_visibility puts them: n bytes of the second record buffer)
    auto d_counts = [&] { return reinterpret_cast<uint8_t *>(s->scratch_b.get()); };
    return host_call(
        s, n, nullptr, 0, n, out_ms,
        [&] {
            int rc = trx_trace_primary_inst_dev(s, view, w, h, whole, sem, s->scratch_a.get(), s->scratch_ia.get(), nullptr);
            if (rc) return rc;
            rc = trx_hit_attributes_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(), nullptr);
            if (rc) return rc;
            if (smooth) {
                rc = trx_shading_normals_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(),
                                                     s->scratch_attr.get(), nullptr);
                if (rc) return rc;
            }
            rc = trx_trace_light_visibility_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps,
                                                s->scratch_a.get(), s->scratch_ia.get(), d_lit(), nullptr);
            if (rc) return rc;
            if (ao_samples != 0) {
                rc = trx_trace_ao_visibility_dev(s, view, w, h, whole, sem, frame0, ao_samples, ao_eps, ao_radius, s->scratch_a.get(),
                                                 s->scratch_ia.get(), d_counts(), nullptr);
                if (rc) return rc;
                rc = trx_ao_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), d_counts(), ao_samples, filter_radius, depth_tol,
                                       normal_cos, d_term(), nullptr);
                if (rc) return rc;
            }
            rc = trx_light_term_dev(s, view, w, h, whole, lights, n_lights, light_samples, s->scratch_a.get(), s->scratch_attr.get(),
                                    d_lit(), ao_samples != 0 ? d_term() : nullptr, ambient, d_value(), nullptr);
            if (rc) return rc;
            if (bounce_samples != 0 && bounce_stride != 0) {
                rc = trx_trace_indirect_sparse_dev(s, view, w, h, bounce_stride, bounce_phase, sem, ray_mask, lights, n_lights, frame0,
                                                   bounce_samples, bounce_eps, shadow_eps, bounce_albedo, s->scratch_a.get(),
                                                   s->scratch_ia.get(), d_low(), nullptr);
                if (rc) return rc;
                const bool filter = filter_levels != 0;
                rc = trx_value_upsample_dev(s, w, h, bounce_stride, bounce_phase, s->scratch_a.get(), s->scratch_attr.get(), d_low(),
                                            filter ? nullptr : d_value(), upsample_radius, bounce_depth_tol, bounce_normal_cos,
                                            filter ? d_indirect() : d_value(), nullptr);
                if (rc) return rc;
                if (filter) {
                    rc = trx_value_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), d_indirect(), d_value(), filter_levels,
                                              bounce_depth_tol, bounce_normal_cos, d_work(), d_value(), nullptr);
                    if (rc) return rc;
                }
            } else if (bounce_samples != 0 && filter_levels == 0) {
                rc = trx_trace_indirect_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, bounce_samples, bounce_eps,
                                            shadow_eps, bounce_albedo, s->scratch_a.get(), s->scratch_ia.get(), d_value(), d_value(), nullptr);
                if (rc) return rc;
            } else if (bounce_samples != 0) {
                rc = trx_trace_indirect_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, bounce_samples, bounce_eps,
                                            shadow_eps, bounce_albedo, s->scratch_a.get(), s->scratch_ia.get(), nullptr, d_indirect(), nullptr);
                if (rc) return rc;
                rc = trx_value_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), d_indirect(), d_value(), filter_levels,
                                          bounce_depth_tol, bounce_normal_cos, d_work(), d_value(), nullptr);
                if (rc) return rc;
            }
            return trx_shade_value_dev(s, d_value(), n, d_rgba(), nullptr);
        },
        [&]() -> int {
            if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, d_rgba(), n * 4, hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

int trx_render_image_lit(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                         const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                         float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                         float normal_cos, uint8_t *out_rgba, float *out_ms) {
    return render_lit(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                      ao_radius, filter_radius, depth_tol, normal_cos, 0u, 0.0f, 0.0f, 0u, 0.0f, 0.0f, 0u, 0u, 0u, out_rgba, out_ms);
}

int trx_render_image_lit_smooth(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                                float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                                float normal_cos, uint8_t *out_rgba, float *out_ms) {
    return render_lit(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                      ao_radius, filter_radius, depth_tol, normal_cos, 0u, 0.0f, 0.0f, 0u, 0.0f, 0.0f, 0u, 0u, 0u, out_rgba, out_ms, true);
}

// what trx_render_image_gi adds to the lit image's refusals (which come first, in their order)
static int check_bounce(const trx_light *lights, uint32_t n_lights, uint32_t light_samples, uint32_t bounce_samples, float bounce_eps,
                        float bounce_albedo) {
    if (int rc = check_lights(lights, n_lights, light_samples)) return rc;
    if (bounce_samples == 0 || bounce_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "bounce_samples %u outside 1..%d", bounce_samples, TRX_MAX_AO_SAMPLES);
    if (!(bounce_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "bounce_eps %g: must be >= 0", (double)bounce_eps);
    if (!std::isfinite(bounce_albedo)) return fail(TRX_ERR_INVALID, "bounce_albedo %g is not finite", (double)bounce_albedo);
    return TRX_OK;
}

int trx_render_image_gi(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                        const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                        float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                        float normal_cos, uint32_t bounce_samples, float bounce_eps, float bounce_albedo, uint8_t *out_rgba,
                        float *out_ms) {
    if (int rc = check_bounce(lights, n_lights, light_samples, bounce_samples, bounce_eps, bounce_albedo)) return rc;
    return render_lit(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                      ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_albedo, 0u, 0.0f, 0.0f, 0u, 0u, 0u,
                      out_rgba, out_ms);
}

int trx_render_image_gi_filtered(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                 const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                                 float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius,
                                 float depth_tol, float normal_cos, uint32_t bounce_samples, float bounce_eps, float bounce_albedo,
                                 uint32_t bounce_filter_levels, float bounce_depth_tol, float bounce_normal_cos, uint8_t *out_rgba,
                                 float *out_ms) {
    if (int rc = check_bounce(lights, n_lights, light_samples, bounce_samples, bounce_eps, bounce_albedo)) return rc;
    if (bounce_filter_levels > TRX_MAX_VALUE_FILTER_LEVELS)
        return fail(TRX_ERR_INVALID, "bounce_filter_levels %u outside 0..%d", bounce_filter_levels, TRX_MAX_VALUE_FILTER_LEVELS);
    if (bounce_filter_levels != 0)
        if (int rc = check_value_filter(bounce_filter_levels, bounce_depth_tol, bounce_normal_cos)) return rc;
    return render_lit(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                      ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_albedo, bounce_filter_levels,
                      bounce_depth_tol, bounce_normal_cos, 0u, 0u, 0u, out_rgba, out_ms);
}

int trx_render_image_gi_sparse(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                               const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                               float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                               float normal_cos, uint32_t bounce_samples, float bounce_eps, float bounce_albedo,
                               uint32_t bounce_filter_levels, float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride,
                               uint32_t bounce_phase, uint32_t bounce_upsample_radius, uint8_t *out_rgba, float *out_ms) {
    if (int rc = check_bounce(lights, n_lights, light_samples, bounce_samples, bounce_eps, bounce_albedo)) return rc;
    if (bounce_filter_levels > TRX_MAX_VALUE_FILTER_LEVELS)
        return fail(TRX_ERR_INVALID, "bounce_filter_levels %u outside 0..%d", bounce_filter_levels, TRX_MAX_VALUE_FILTER_LEVELS);
    // (the upsample looks at the two tolerances whatever the levels)
    if (int rc = check_value_upsample(bounce_stride, bounce_phase, bounce_upsample_radius, bounce_depth_tol, bounce_normal_cos)) return rc;
    return render_lit(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                      ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_albedo, bounce_filter_levels,
                      bounce_depth_tol, bounce_normal_cos, bounce_stride, bounce_phase, bounce_upsample_radius, out_rgba, out_ms);
}

// ---- the colour image (include/trx.h, "materials") ---------------------------------------------------------------------------------

// (the scene's tables are swapped under s->mu and, once set, only ever replaced: what holds here holds when the pass reads them)
static int need_materials(trx_scene *s) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->materials) return fail(TRX_ERR_INVALID, "the scene has no materials (trx_scene_set_materials)");
    return TRX_OK;
}

int trx_material_compose_dev(trx_scene *s, const trx_hit *d_primary, const float *d_direct, const float *d_indirect_rgb, uint64_t n,
                             float *d_colour_rgb, void *stream) {
    if (!s || !d_primary || !d_direct || !d_colour_rgb) return fail(TRX_ERR_INVALID, "null argument");
    if (n == 0 || n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "n_records %llu outside 1..2^31 - 1", (unsigned long long)n);
    if (int rc = need_materials(s)) return rc;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        ComposeParams p;
        std::memset(&p, 0, sizeof(p));
        p.primary = d_primary;
        p.direct = d_direct;
        p.indirect = d_indirect_rgb;
        p.out = d_colour_rgb;
        p.materials = s->materials.get(); // (under s->mu: enqueue_image holds it)
        p.tri_material = s->tri_material.get();
        p.n_items = (uint32_t)n;
        p.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull);
        HIP_TRY(launch_compose(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

int trx_shade_rgb_dev(trx_scene *s, const float *d_colour_rgb, uint64_t n, uint8_t *d_rgba, void *stream) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (n == 0) return TRX_OK;
    if (!d_colour_rgb || !d_rgba) return fail(TRX_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_rgba) & 3u) return fail(TRX_ERR_INVALID, "d_rgba is not 4-byte aligned");
    if (n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "n_records %llu beyond 2^31 - 1", (unsigned long long)n);
    return enqueue_image(s, (hipStream_t)stream, true, [&]() -> int {
        ShadeRgbParams p;
        std::memset(&p, 0, sizeof(p));
        p.thr = s->image_thr.get();
        p.colour = d_colour_rgb;
        p.rgba = d_rgba;
        p.n_items = (uint32_t)n;
        HIP_TRY(launch_shade_rgb(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

// ---- the textured albedo (include/trx.h, "texture coordinates and albedo textures") ---------------------------------------------------

// Both passes take a launch slot (enqueue_image): a swap of the materials, the texcoords or the texture set, and a refit,
// called afterwards wait for the slot's `done` event.
int trx_surface_albedo_dev(trx_scene *s, const trx_hit *d_hits, const trx_hit_attr *d_attr, uint64_t n, float *d_albedo_rgb, void *stream) {
    if (!s || !d_hits || !d_attr || !d_albedo_rgb) return fail(TRX_ERR_INVALID, "null argument");
    if (n == 0 || n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "n_records %llu outside 1..2^31 - 1", (unsigned long long)n);
    if (int rc = need_materials(s)) return rc;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        SurfaceAlbedoParams p;
        std::memset(&p, 0, sizeof(p));
        p.hits = d_hits;
        p.attr = d_attr;
        p.out = d_albedo_rgb;
        p.materials = s->materials.get(); // (under s->mu: enqueue_image holds it)
        p.tri_material = s->tri_material.get();
        p.tex.texcoords = s->texcoords.get(); // (null without a table: the plain albedo)
        if (s->material_texture) {
            p.tex.descs = s->tex_descs.get();
            p.tex.texels = s->texels.get();
            p.tex.material_texture = s->material_texture.get();
            p.tex.srgb = s->tex_srgb.get();
        }
        p.n_items = (uint32_t)n;
        p.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull);
        HIP_TRY(launch_surface_albedo(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

int trx_albedo_compose_dev(trx_scene *s, const trx_hit *d_primary, const float *d_albedo_rgb, const float *d_direct,
                           const float *d_indirect_rgb, uint64_t n, float *d_colour_rgb, void *stream) {
    if (!s || !d_primary || !d_albedo_rgb || !d_direct || !d_colour_rgb) return fail(TRX_ERR_INVALID, "null argument");
    if (n == 0 || n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "n_records %llu outside 1..2^31 - 1", (unsigned long long)n);
    if (int rc = need_materials(s)) return rc;
    return enqueue_image(s, (hipStream_t)stream, false, [&]() -> int {
        AlbedoComposeParams p;
        std::memset(&p, 0, sizeof(p));
        p.primary = d_primary;
        p.albedo = d_albedo_rgb;
        p.direct = d_direct;
        p.indirect = d_indirect_rgb;
        p.out = d_colour_rgb;
        p.materials = s->materials.get(); // (under s->mu: enqueue_image holds it)
        p.tri_material = s->tri_material.get();
        p.n_items = (uint32_t)n;
        p.n_tris = (uint32_t)std::min<uint64_t>(s->n_tris, 0xffffffffull);
        HIP_TRY(launch_albedo_compose(p, (hipStream_t)stream));
        return TRX_OK;
    });
}

} // extern "C"

// trx_render_image_colour (emitter_eps null) and trx_render_image_colour_emitters (include/trx.h, "emitters": emitter_eps set -
// n_lights may be 0, the indirect pass runs in its emitter mode, and the emitter light pass adds to the planes the indirect
// term ends in before the compose); smooth (trx_render_image_colour_smooth): render_lit's statement of it
static int render_colour(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                         const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                         float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                         float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t filter_levels, float bounce_depth_tol,
                         float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase, uint32_t upsample_radius,
                         uint32_t emitter_samples, const float *emitter_eps, uint8_t *out_rgba, float *out_ms, bool smooth = false,
                         bool textured = false) {
    // render_lit's refusals in its order, then the bounce's, the filter's and the upsample's where those steps run
    // (no light at all - the emitter form alone: V is what the light term gives for this one light of intensity 0)
    const trx_light none{TRX_LIGHT_DIRECTIONAL, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, {0u, 0u}};
    const bool unlit = emitter_eps && n_lights == 0;
    if (unlit) {
        if (light_samples == 0 || light_samples > TRX_MAX_AO_SAMPLES)
            return fail(TRX_ERR_INVALID, "n_samples %u outside 1..%d", light_samples, TRX_MAX_AO_SAMPLES);
    } else if (int rc = check_lights(lights, n_lights, light_samples)) return rc;
    if (ray_mask > 0xffu) return fail(TRX_ERR_INVALID, "ray_mask 0x%x outside 0..255", ray_mask);
    if (!(shadow_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "shadow_eps %g: must be >= 0", (double)shadow_eps);
    if (!std::isfinite(ambient)) return fail(TRX_ERR_INVALID, "ambient %g is not finite", (double)ambient);
    if (ao_samples > TRX_MAX_AO_SAMPLES) return fail(TRX_ERR_INVALID, "ao_samples %u outside 0..%d", ao_samples, TRX_MAX_AO_SAMPLES);
    if (ao_samples != 0) {
        if (!(ao_radius > 0.0f)) return fail(TRX_ERR_INVALID, "ao_radius %g: must be > 0 (+inf allowed)", (double)ao_radius);
        if (int rc = check_filter(filter_radius, depth_tol, normal_cos)) return rc;
    }
    if (sem & ~7u) return fail(TRX_ERR_INVALID, "unknown semantics bits 0x%x", sem);
    if (int rc = check_image(w, h)) return rc;
    if (!s || !view) return fail(TRX_ERR_INVALID, "null argument");
    if (bounce_samples > TRX_MAX_AO_SAMPLES)
        return fail(TRX_ERR_INVALID, "bounce_samples %u outside 0..%d", bounce_samples, TRX_MAX_AO_SAMPLES);
    const bool sparse = bounce_samples != 0 && bounce_stride > 1u, filter = bounce_samples != 0 && filter_levels != 0;
    if (bounce_samples != 0) {
        if (!(bounce_eps >= 0.0f)) return fail(TRX_ERR_INVALID, "bounce_eps %g: must be >= 0", (double)bounce_eps);
        if (filter_levels > TRX_MAX_VALUE_FILTER_LEVELS)
            return fail(TRX_ERR_INVALID, "bounce_filter_levels %u outside 0..%d", filter_levels, TRX_MAX_VALUE_FILTER_LEVELS);
        if (filter)
            if (int rc = check_value_filter(filter_levels, bounce_depth_tol, bounce_normal_cos)) return rc;
        if (int rc = check_sparse(bounce_stride, bounce_phase, 0u)) return rc;
        if (sparse)
            if (int rc = check_value_upsample(bounce_stride, bounce_phase, upsample_radius, bounce_depth_tol, bounce_normal_cos)) return rc;
    }
    if (emitter_eps) {
        if (emitter_samples == 0 || emitter_samples > TRX_MAX_AO_SAMPLES)
            return fail(TRX_ERR_INVALID, "emitter_samples %u outside 1..%d", emitter_samples, TRX_MAX_AO_SAMPLES);
        if (int rc = check_emitter_eps(*emitter_eps)) return rc;
    }
    if (int rc = need_materials(s)) return rc;
    if (smooth)
        if (int rc = need_vertex_normals(s)) return rc;
    const uint64_t n = (uint64_t)w * h;
    const trx_shard whole{0, 1, 0, 0};
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (host_call takes it again: the image scratch is under it too)
    HIP_TRY(hipSetDevice(s->device));
    if (emitter_eps) { // (no table yet, or a stale one: built here; every call that stales it holds host_mu)
        bool build;
        {
            std::lock_guard<std::mutex> lock(s->mu);
            build = s->n_emitters == 0 || s->emitters_stale;
        }
        if (build) if (int rc = trx_scene_build_emitters(s, nullptr)) return rc;
    }
    // the image scratch: the AO filter's terms, the image, the light term's values, two sets of three planes (the indirect
    // term's steps alternate between them: a low grid holds at most n cells), the value filter's work plane, the lights' planes
    // (textured: three albedo planes more, ahead of the lights' planes)
    const uint64_t lit_at = n * 4 * (textured ? 13 : 10);
    HIP_TRY(s->scratch_img.grow(lit_at + n * (unlit ? 1u : n_lights)));
    auto d_term = [&] { return reinterpret_cast<trx_ao_term *>(s->scratch_img.get()); };
    auto d_rgba = [&] { return s->scratch_img.get() + n * 4; };
    auto d_value = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 8); };
    auto d_a = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 12); };
    auto d_b = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 24); };
    auto d_work = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 36); };
    auto d_albedo = [&] { return reinterpret_cast<float *>(s->scratch_img.get() + n * 40); }; // (textured only)
    auto d_lit = [&] { return s->scratch_img.get() + lit_at; };
    auto d_counts = [&] { return reinterpret_cast<uint8_t *>(s->scratch_b.get()); };
    return host_call(
        s, n, nullptr, 0, n, out_ms,
        [&] {
            int rc = trx_trace_primary_inst_dev(s, view, w, h, whole, sem, s->scratch_a.get(), s->scratch_ia.get(), nullptr);
            if (rc) return rc;
            rc = trx_hit_attributes_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(), nullptr);
            if (rc) return rc;
            if (smooth) {
                rc = trx_shading_normals_primary_dev(s, view, w, h, whole, s->scratch_a.get(), s->scratch_ia.get(), s->scratch_attr.get(),
                                                     s->scratch_attr.get(), nullptr);
                if (rc) return rc;
            }
            if (textured) { // (u and v are the attribute pass's with or without the shading normals)
                rc = trx_surface_albedo_dev(s, s->scratch_a.get(), s->scratch_attr.get(), n, d_albedo(), nullptr);
                if (rc) return rc;
            }
            if (unlit) HIP_TRY(hipMemsetAsync(d_lit(), 0, n, nullptr)); // (a light of intensity 0 adds +0 whatever its plane counts)
            else rc = trx_trace_light_visibility_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps,
                                                     s->scratch_a.get(), s->scratch_ia.get(), d_lit(), nullptr);
            if (rc) return rc;
            if (ao_samples != 0) {
                rc = trx_trace_ao_visibility_dev(s, view, w, h, whole, sem, frame0, ao_samples, ao_eps, ao_radius, s->scratch_a.get(),
                                                 s->scratch_ia.get(), d_counts(), nullptr);
                if (rc) return rc;
                rc = trx_ao_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), d_counts(), ao_samples, filter_radius, depth_tol,
                                       normal_cos, d_term(), nullptr);
                if (rc) return rc;
            }
            rc = trx_light_term_dev(s, view, w, h, whole, unlit ? &none : lights, unlit ? 1u : n_lights, light_samples, s->scratch_a.get(),
                                    s->scratch_attr.get(), d_lit(), ao_samples != 0 ? d_term() : nullptr, ambient, d_value(), nullptr);
            if (rc) return rc;
            float *planes = nullptr; // the indirect term's three full-resolution planes, or none
            if (bounce_samples != 0) {
                float *other = d_b();
                planes = d_a();
                // (textured: one entry point for the four modes - stride 1 is its dense pass)
                auto textured_pass = [&](uint32_t stride, uint32_t phase) {
                    return trx_trace_indirect_rgb_textured_dev(s, view, w, h, whole, stride, phase, sem, ray_mask, lights, n_lights, frame0, bounce_samples,
                                                               bounce_eps, shadow_eps, emitter_eps ? 1u : 0u, emitter_eps ? *emitter_eps : 0.0f,
                                                               s->scratch_a.get(), s->scratch_ia.get(), planes, nullptr);
                };
                if (sparse) {
                    rc = textured ? textured_pass(bounce_stride, bounce_phase)
                         : emitter_eps ? trx_trace_indirect_rgb_emitters_sparse_dev(s, view, w, h, bounce_stride, bounce_phase, sem, ray_mask, lights,
                                                                                  n_lights, frame0, bounce_samples, bounce_eps, shadow_eps,
                                                                                  *emitter_eps, s->scratch_a.get(), s->scratch_ia.get(), planes, nullptr)
                                     : trx_trace_indirect_rgb_sparse_dev(s, view, w, h, bounce_stride, bounce_phase, sem, ray_mask, lights, n_lights,
                                                                         frame0, bounce_samples, bounce_eps, shadow_eps, s->scratch_a.get(),
                                                                         s->scratch_ia.get(), planes, nullptr);
                    if (rc) return rc;
                    const uint64_t n_lo = (uint64_t)((w + bounce_stride - 1u) / bounce_stride) * ((h + bounce_stride - 1u) / bounce_stride);
                    for (uint64_t c = 0; c < 3; c++) {
                        rc = trx_value_upsample_dev(s, w, h, bounce_stride, bounce_phase, s->scratch_a.get(), s->scratch_attr.get(),
                                                    planes + c * n_lo, nullptr, upsample_radius, bounce_depth_tol, bounce_normal_cos,
                                                    other + c * n, nullptr);
                        if (rc) return rc;
                    }
                    std::swap(planes, other);
                } else {
                    rc = textured ? textured_pass(1u, 0u)
                         : emitter_eps ? trx_trace_indirect_rgb_emitters_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, bounce_samples,
                                                                           bounce_eps, shadow_eps, *emitter_eps, s->scratch_a.get(),
                                                                           s->scratch_ia.get(), planes, nullptr)
                                     : trx_trace_indirect_rgb_dev(s, view, w, h, whole, sem, ray_mask, lights, n_lights, frame0, bounce_samples,
                                                                  bounce_eps, shadow_eps, s->scratch_a.get(), s->scratch_ia.get(), planes, nullptr);
                    if (rc) return rc;
                }
                if (filter) {
                    for (uint64_t c = 0; c < 3; c++) {
                        rc = trx_value_filter_dev(s, w, h, s->scratch_a.get(), s->scratch_attr.get(), planes + c * n, nullptr, filter_levels,
                                                  bounce_depth_tol, bounce_normal_cos, d_work(), other + c * n, nullptr);
                        if (rc) return rc;
                    }
                    std::swap(planes, other);
                }
            }
            // (the colour lands in the planes the indirect term ends in - the compose may run in place - or in the first set)
            float *colour = planes ? planes : d_a();
            if (emitter_eps) { // the emitter light pass at full resolution, unfiltered: the planes so far its base and its output
                rc = trx_trace_emitter_light_dev(s, view, w, h, whole, sem, ray_mask, frame0, emitter_samples, shadow_eps, *emitter_eps,
                                                 s->scratch_a.get(), s->scratch_ia.get(), planes, colour, nullptr);
                if (rc) return rc;
                planes = colour;
            }
            rc = textured ? trx_albedo_compose_dev(s, s->scratch_a.get(), d_albedo(), d_value(), planes, n, colour, nullptr)
                          : trx_material_compose_dev(s, s->scratch_a.get(), d_value(), planes, n, colour, nullptr);
            if (rc) return rc;
            return trx_shade_rgb_dev(s, colour, n, d_rgba(), nullptr);
        },
        [&]() -> int {
            if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, d_rgba(), n * 4, hipMemcpyDeviceToHost));
            return TRX_OK;
        });
}

extern "C" {

int trx_render_image_colour(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                            const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                            float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                            float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t filter_levels, float bounce_depth_tol,
                            float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase, uint32_t upsample_radius,
                            uint8_t *out_rgba, float *out_ms) {
    return render_colour(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                         ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, filter_levels, bounce_depth_tol,
                         bounce_normal_cos, bounce_stride, bounce_phase, upsample_radius, 0u, nullptr, out_rgba, out_ms);
}

int trx_render_image_colour_smooth(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                   const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                                   float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius, float depth_tol,
                                   float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t filter_levels, float bounce_depth_tol,
                                   float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase, uint32_t upsample_radius,
                                   uint8_t *out_rgba, float *out_ms) {
    return render_colour(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                         ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, filter_levels, bounce_depth_tol,
                         bounce_normal_cos, bounce_stride, bounce_phase, upsample_radius, 0u, nullptr, out_rgba, out_ms, true);
}

int trx_render_image_colour_emitters(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                     const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                                     float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius,
                                     float depth_tol, float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t filter_levels,
                                     float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase,
                                     uint32_t upsample_radius, uint32_t emitter_samples, float emitter_eps, uint8_t *out_rgba,
                                     float *out_ms) {
    return render_colour(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                         ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, filter_levels, bounce_depth_tol,
                         bounce_normal_cos, bounce_stride, bounce_phase, upsample_radius, emitter_samples, &emitter_eps, out_rgba, out_ms);
}

// trx_render_image_colour / _smooth / _emitters in one, with the textured albedo (include/trx.h, "texture coordinates and
// albedo textures"): render_colour's `textured`
int trx_render_image_colour_textured(trx_scene *s, const trx_view *view, uint32_t w, uint32_t h, uint32_t sem, uint32_t ray_mask,
                                     const trx_light *lights, uint32_t n_lights, uint32_t frame0, uint32_t light_samples, float shadow_eps,
                                     float ambient, uint32_t ao_samples, float ao_eps, float ao_radius, uint32_t filter_radius,
                                     float depth_tol, float normal_cos, uint32_t bounce_samples, float bounce_eps, uint32_t filter_levels,
                                     float bounce_depth_tol, float bounce_normal_cos, uint32_t bounce_stride, uint32_t bounce_phase,
                                     uint32_t upsample_radius, uint32_t emitter_samples, float emitter_eps, uint32_t smooth,
                                     uint8_t *out_rgba, float *out_ms) {
    if (smooth > 1u) return fail(TRX_ERR_INVALID, "smooth %u: must be 0 or 1", smooth);
    return render_colour(s, view, w, h, sem, ray_mask, lights, n_lights, frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps,
                         ao_radius, filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps, filter_levels, bounce_depth_tol,
                         bounce_normal_cos, bounce_stride, bounce_phase, upsample_radius, emitter_samples,
                         emitter_samples ? &emitter_eps : nullptr, out_rgba, out_ms, smooth != 0u, true);
}

} // extern "C"
