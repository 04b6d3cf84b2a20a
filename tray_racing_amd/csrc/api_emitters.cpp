// api_emitters.cpp - the emitter table (include/trx.h, "emitters"): trx_scene_build_emitters finds the scene's emissive
// (instance, triangle) pairs on the host, has k_emitter_build (kernels.hip) write their world-space records, reads them back
// and builds the selection table in binary64; trx_scene_get_emitters hands the table out; trx_debug_emitter_select runs the
// device's selection function over caller-given values.  The passes that use the table are in api_ao.cpp.
#include "api_internal.h"
#include "build_rules.h"

#include <map>

namespace {

// (api.cpp's rule for a table swapped out under s->mu: freed once the wait for the kernels that may read it succeeded, kept otherwise)
template <typename T>
hipError_t retire(DevBuf<T> &old, hipError_t waited) {
    if (waited == hipSuccess) old.reset();
    else (void)old.release();
    return waited;
}

bool emits(const trx_material &m) { return m.emission[0] > 0.0f || m.emission[1] > 0.0f || m.emission[2] > 0.0f; }

// The emissive triangles reachable from node `start` of the BLAS segment that begins at `seg`, ascending by prim.  The node
// buffer passed trx_scene_create's validation; the step cap and the range tests are for a buffer a refit rewrote.
int blas_emitters(const std::vector<CwbvhNode> &nodes, uint32_t seg, uint32_t start, uint32_t tlas_start, const std::vector<uint8_t> &emissive,
                  std::vector<uint32_t> &out) {
    std::vector<uint32_t> stack{start};
    uint64_t steps = 0;
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        if (i >= tlas_start || ++steps > nodes.size()) return fail(TRX_ERR_FORMAT, "emitters: node %u leaves its BLAS", i);
        const CwbvhNode &n = nodes[i];
        uint32_t rank = 0;
        for (int s = 0; s < 8; s++) {
            const uint8_t m = n.child_meta[s];
            if (m == 0) continue;
            if ((m & 0x18) == 0x18) {
                stack.push_back(seg + n.child_base_idx + rank++);
                continue;
            }
            const uint64_t first = (uint64_t)n.primitive_base_idx + (m & 0x1fu), cnt = leaf_count(m);
            if (first + cnt > emissive.size()) return fail(TRX_ERR_FORMAT, "emitters: node %u references triangle %llu", i, (unsigned long long)(first + cnt - 1));
            for (uint64_t j = first; j < first + cnt; j++)
                if (emissive[j]) out.push_back((uint32_t)j);
        }
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return TRX_OK;
}

} // namespace

int trxapi::need_emitters(const trx_scene *s) {
    if (!s->emitters || s->n_emitters == 0) return fail(TRX_ERR_INVALID, "the scene has no emitter table (trx_scene_build_emitters)");
    if (s->emitters_stale)
        return fail(TRX_ERR_INVALID, "the emitter table is stale: materials, triangles or instances changed since trx_scene_build_emitters");
    return TRX_OK;
}

int trxapi::check_emitter_eps(float emitter_eps) {
    if (!(emitter_eps >= 0.0f && emitter_eps < 1.0f)) return fail(TRX_ERR_INVALID, "emitter_eps %g: must be in [0, 1)", (double)emitter_eps);
    return TRX_OK;
}

extern "C" {

int trx_scene_build_emitters(trx_scene *s, uint32_t *out_n) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    // (every call that changes what the table is made of - materials, refit, instances - holds host_mu as well)
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    if (s->h_materials.empty()) return fail(TRX_ERR_INVALID, "the scene has no materials (trx_scene_set_materials)");
    if (s->n_tris >= 0xffffffffull) return fail(TRX_ERR_INVALID, "emitters: the scene has too many triangles");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint2> pairs;
    try {
        std::vector<uint8_t> emissive(s->n_tris);
        for (uint64_t i = 0; i < s->n_tris; i++) emissive[i] = emits(s->h_materials[s->h_tri_material[i]]) ? 1 : 0;
        if (!s->tlas) {
            for (uint64_t i = 0; i < s->n_tris && pairs.size() <= TRX_MAX_EMITTERS; i++)
                if (emissive[i]) pairs.push_back(make_uint2(0xffffffffu, (uint32_t)i));
        } else if (std::find(emissive.begin(), emissive.end(), 1) != emissive.end()) {
            // a stream of its own for the read-back: the null stream would wait for the scene's resident ray services
            Stream rd;
            HIP_TRY(rd.create(hipStreamNonBlocking));
            std::vector<CwbvhNode> nodes(s->n_nodes);
            HIP_TRY(hipMemcpyAsync(nodes.data(), s->nodes.get(), s->n_nodes * TRX_NODE_BYTES, hipMemcpyDeviceToHost, rd.get()));
            HIP_TRY(hipStreamSynchronize(rd.get()));
            std::map<uint32_t, std::vector<uint32_t>> of_entry; // instances that share an entry node share its list
            for (uint32_t k = 0; k < s->n_inst && pairs.size() <= TRX_MAX_EMITTERS; k++) {
                const uint32_t seg = s->h_inst[k], start = seg + (s->h_inst_entry.empty() ? 0u : s->h_inst_entry[k]);
                auto it = of_entry.find(start);
                if (it == of_entry.end()) {
                    std::vector<uint32_t> list;
                    if (int rc = blas_emitters(nodes, seg, start, s->tlas_start, emissive, list)) return rc;
                    it = of_entry.emplace(start, std::move(list)).first;
                }
                for (uint32_t prim : it->second) {
                    pairs.push_back(make_uint2(k, prim));
                    if (pairs.size() > TRX_MAX_EMITTERS) break;
                }
            }
        }
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    if (pairs.empty()) return fail(TRX_ERR_INVALID, "the scene has no emitters: no material of a triangle has an emission component > 0");
    if (pairs.size() > TRX_MAX_EMITTERS) return fail(TRX_ERR_INVALID, "more than TRX_MAX_EMITTERS (%u) emitters", TRX_MAX_EMITTERS);
    const uint32_t n = (uint32_t)pairs.size();
    // the records: the pairs and (as the refit does) the host copy of the object-to-world matrices uploaded, one kernel
    const bool xf = s->tlas && !s->inst_o2w.empty();
    DevBuf<uint2> d_pairs;
    DevBuf<float> d_o2w;
    DevBuf<float4> fresh;
    DevBuf<float> fresh_cdf;
    HIP_TRY(d_pairs.alloc(n));
    if (xf) HIP_TRY(d_o2w.alloc((uint64_t)s->n_inst * 16));
    HIP_TRY(fresh.alloc((uint64_t)n * 4));
    HIP_TRY(fresh_cdf.alloc(std::max<uint32_t>(n - 1u, 1u)));
    Stream st;
    HIP_TRY(st.create(hipStreamNonBlocking));
    std::vector<float> rec, cdf;
    try {
        rec.resize((size_t)n * 16);
        cdf.resize(n - 1u);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    HIP_TRY(hipMemcpyAsync(d_pairs.get(), pairs.data(), (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, st.get()));
    if (xf) HIP_TRY(hipMemcpyAsync(d_o2w.get(), s->inst_o2w.data(), (size_t)s->n_inst * 64, hipMemcpyHostToDevice, st.get()));
    EmitterBuildParams bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.tris = s->tris.get();
    bp.o2w = xf ? d_o2w.get() : nullptr;
    bp.pairs = d_pairs.get();
    bp.tri_material = s->tri_material.get();
    bp.out = fresh.get();
    bp.n = n;
    bp.n_tris = (uint32_t)s->n_tris;
    bp.n_inst = s->n_inst;
    HIP_TRY(launch_emitter_build(bp, st.get()));
    HIP_TRY(hipMemcpyAsync(rec.data(), fresh.get(), (size_t)n * 64, hipMemcpyDeviceToHost, st.get()));
    HIP_TRY(hipStreamSynchronize(st.get()));
    // the selection table, in binary64 and in index order (include/trx.h)
    std::vector<double> wj(n);
    double W = 0.0;
    for (uint32_t j = 0; j < n; j++) {
        const float *r = &rec[(size_t)j * 16];
        uint32_t m;
        std::memcpy(&m, &r[7], 4);
        if (m >= s->h_materials.size()) return fail(TRX_ERR_NO_DEVICE, "emitters: the device wrote record %u with material %u", j, m);
        const trx_material &mat = s->h_materials[m];
        const double nx = r[12], ny = r[13], nz = r[14];
        wj[j] = std::sqrt(nx * nx + ny * ny + nz * nz) * ((double)mat.emission[0] + (double)mat.emission[1] + (double)mat.emission[2]);
        W += wj[j];
    }
    double run = 0.0;
    for (uint32_t j = 0; j < n; j++) {
        const double p = W == 0.0 ? 1.0 / (double)n : 0.5 * wj[j] / W + 0.5 / (double)n;
        const float P = (float)p;
        rec[(size_t)j * 16 + 3] = (float)(1.0 / (3.14159265358979323846 * (double)P));
        run += p;
        if (j + 1 < n) cdf[j] = (float)run;
    }
    HIP_TRY(hipMemcpyAsync(fresh.get(), rec.data(), (size_t)n * 64, hipMemcpyHostToDevice, st.get()));
    if (n > 1) HIP_TRY(hipMemcpyAsync(fresh_cdf.get(), cdf.data(), (size_t)(n - 1u) * sizeof(float), hipMemcpyHostToDevice, st.get()));
    else HIP_TRY(hipMemsetAsync(fresh_cdf.get(), 0, sizeof(float), st.get()));
    HIP_TRY(hipStreamSynchronize(st.get()));
    // Swapped under the launch mutex; the old tables are freed once every launch slot's last kernel has finished -
    // trx_scene_set_materials' statement: a pass enqueued before this call uses the old table in full.
    DevBuf<float4> old;
    DevBuf<float> old_cdf;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        old = std::move(s->emitters);
        old_cdf = std::move(s->emitter_cdf);
        s->emitters = std::move(fresh);
        s->emitter_cdf = std::move(fresh_cdf);
        s->h_emitters.swap(rec);
        s->h_emitter_cdf.swap(cdf);
        s->n_emitters = n;
        s->emitters_stale = false;
        if (old)
            for (Slot &sl : s->slots)
                if (sl.used && !sl.pinned && sl.done && e == hipSuccess) e = hipEventSynchronize(sl.done.get());
    }
    (void)retire(old_cdf, e);
    if (retire(old, e) != hipSuccess) // (the old tables are kept rather than freed under a kernel that may still read them)
        return fail(TRX_ERR_NO_DEVICE, "waiting for the scene's launches failed: %s", hipGetErrorString(e));
    if (out_n) *out_n = n;
    return TRX_OK;
}

int trx_scene_get_emitters(const trx_scene *s, float *out_records, uint32_t *inout_n, float *out_c) {
    if (!s || !out_records || !inout_n || !out_c) return fail(TRX_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<trx_scene *>(s)->mu);
    if (int rc = need_emitters(s)) return rc;
    if (*inout_n < s->n_emitters) return fail(TRX_ERR_INVALID, "room for %u emitters, the scene has %u", *inout_n, s->n_emitters);
    std::memcpy(out_records, s->h_emitters.data(), (size_t)s->n_emitters * 64);
    if (s->n_emitters > 1) std::memcpy(out_c, s->h_emitter_cdf.data(), (size_t)(s->n_emitters - 1u) * sizeof(float));
    *inout_n = s->n_emitters;
    return TRX_OK;
}

int trx_debug_emitter_select(trx_scene *s, const float *d_u0, uint64_t n, uint32_t *d_j) {
    if (!s || !d_u0 || !d_j) return fail(TRX_ERR_INVALID, "null argument");
    if (n > 0x7fffffffull) return fail(TRX_ERR_INVALID, "n %llu", (unsigned long long)n);
    HIP_TRY(hipSetDevice(s->device));
    {
        std::lock_guard<std::mutex> lock(s->mu);
        if (int rc = need_emitters(s)) return rc;
        Slot *slot = nullptr;
        if (int rc = acquire_slot(s, nullptr, slot)) return rc;
        EmitterSelectParams p;
        p.cdf = s->emitter_cdf.get();
        p.u0 = d_u0;
        p.j = d_j;
        p.n_emitters = s->n_emitters;
        p.n = (uint32_t)n;
        slot->last_stream = nullptr;
        slot->last_use = ++s->launches;
        HIP_TRY(launch_emitter_select(p, nullptr));
        HIP_TRY(hipEventRecord(slot->done.get(), nullptr));
        slot->used = true;
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return TRX_OK;
}

} // extern "C"
