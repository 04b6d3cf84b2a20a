// api_refit.cpp - trx_scene_refit / trx_scene_refit_dev / trx_scene_read_nodes / trx_refit_nodes (include/trx.h): new
// vertices for a scene whose topology stays, every node's frame and child boxes recomputed.  The per-node rule lives in
// refit_gpu.h (one __host__ __device__ function for the host twin here and the kernels of refit_gpu.cpp); this file
// holds the schedule (nodes by height), the validation, and the device driver with its ordering against the scene's
// launches and ray services.
#include "api_internal.h"
#include "refit_gpu.h"

namespace trx {

int refit_topology(const CwbvhNode *nodes, uint64_t n_nodes, const uint32_t *inst, uint32_t n_inst, uint32_t tlas_start,
                   const uint32_t *entry, RefitTopology &topo, const char **why) {
    const bool tlas = n_inst > 0;
    topo.seg_base.assign(n_nodes, 0u);
    if (tlas) {
        std::vector<uint32_t> seg(inst, inst + n_inst);
        std::sort(seg.begin(), seg.end());
        seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
        for (uint64_t i = 0; i < n_nodes; i++) {
            if (i >= tlas_start) {
                topo.seg_base[i] = tlas_start;
            } else {
                auto it = std::upper_bound(seg.begin(), seg.end(), (uint32_t)i);
                topo.seg_base[i] = it == seg.begin() ? 0u : *(it - 1);
            }
        }
    }
    // the nodes whose boxes node i reads: its inner children, and for a TLAS node the entry nodes of its leaf primitives
    auto deps = [&](uint32_t i, uint32_t *out) -> int {
        const CwbvhNode &n = nodes[i];
        const bool in_tlas = tlas && i >= tlas_start;
        int k = 0;
        uint32_t rank = 0;
        for (int s = 0; s < 8; s++) {
            const uint8_t m = n.child_meta[s];
            if (m == 0) continue;
            if ((m & 0x18) == 0x18) {
                out[k++] = topo.seg_base[i] + n.child_base_idx + rank++;
            } else if (in_tlas) {
                const uint32_t first = n.primitive_base_idx + (m & 0x1fu), cnt = leaf_count(m);
                for (uint32_t j = first; j < first + cnt; j++) out[k++] = inst[j] + (entry ? entry[j] : 0u);
            }
        }
        return k;
    };
    // heights by an explicit depth-first walk (a tree may be deep; a malformed one may loop)
    constexpr uint32_t kUnseen = 0xffffffffu, kOpen = 0xfffffffeu;
    std::vector<uint32_t> height(n_nodes, kUnseen);
    struct Frame {
        uint32_t node;
        int n, next;
        uint32_t h;
        uint32_t dep[8 + 24];
    };
    std::vector<Frame> stack;
    uint32_t max_h = 0;
    for (uint64_t root = 0; root < n_nodes; root++) {
        if (height[root] != kUnseen) continue;
        stack.push_back(Frame{(uint32_t)root, 0, 0, 0, {}});
        stack.back().n = deps((uint32_t)root, stack.back().dep);
        height[root] = kOpen;
        while (!stack.empty()) {
            Frame &f = stack.back();
            if (f.next < f.n) {
                const uint32_t d = f.dep[f.next++];
                if (height[d] == kOpen) {
                    *why = "the node references form a cycle";
                    return TRX_ERR_FORMAT;
                }
                if (height[d] == kUnseen) {
                    height[d] = kOpen;
                    Frame g{d, 0, 0, 0, {}};
                    g.n = deps(d, g.dep);
                    stack.push_back(g); // (invalidates f)
                } else {
                    f.h = std::max(f.h, height[d] + 1u);
                }
                continue;
            }
            const uint32_t node = f.node, h = f.h;
            stack.pop_back();
            height[node] = h;
            max_h = std::max(max_h, h);
            if (!stack.empty()) stack.back().h = std::max(stack.back().h, h + 1u);
        }
    }
    // counting sort by height, node ids ascending inside a level
    topo.level_start.assign((size_t)max_h + 2, 0u);
    for (uint64_t i = 0; i < n_nodes; i++) topo.level_start[height[i] + 1]++;
    for (size_t l = 1; l < topo.level_start.size(); l++) topo.level_start[l] += topo.level_start[l - 1];
    topo.order.assign(n_nodes, 0u);
    std::vector<uint32_t> at(topo.level_start.begin(), topo.level_start.end() - 1);
    for (uint64_t i = 0; i < n_nodes; i++) topo.order[at[height[i]]++] = (uint32_t)i;
    return TRX_OK;
}

} // namespace trx

namespace trxapi {

uint64_t refit_state_bytes(const trx_scene *s) {
    const RefitState &r = s->refit;
    uint64_t b = r.result.count() * sizeof(RefitResult);
    if (r.have_topology) b += s->n_nodes * (2 * sizeof(uint32_t) + 6 * sizeof(float));
    return b + r.o2w.count() * sizeof(float);
}

} // namespace trxapi

namespace {

// entry node k must lie inside the BLAS segment that starts at inst[k] (as trx_scene_set_instance_entry_nodes checks)
int validate_entries(const uint32_t *inst, uint32_t n_inst, uint32_t tlas_start, const uint32_t *entry) {
    std::vector<uint32_t> seg(inst, inst + n_inst);
    std::sort(seg.begin(), seg.end());
    seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
    for (uint32_t k = 0; k < n_inst; k++) {
        auto it = std::upper_bound(seg.begin(), seg.end(), inst[k]);
        const uint32_t seg_end = it == seg.end() ? tlas_start : *it;
        if ((uint64_t)inst[k] + entry[k] >= seg_end)
            return fail(TRX_ERR_FORMAT, "instance %u: entry node %u leaves its BLAS [%u, %u)", k, entry[k], inst[k], seg_end);
    }
    return TRX_OK;
}

bool all_finite(const float *v, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// Stops the scene's ray services and keeps them stopped while the holder lives: their resident kernels read the node
// and triangle buffers outside stream order.  A trx_traverse1 caller that arrives meanwhile waits on the service's mutex
// and restarts it lazily afterwards (its request stays in the ring).
struct ServicesHeld {
    std::unique_lock<std::mutex> create;
    std::vector<std::unique_lock<std::mutex>> held;
    explicit ServicesHeld(trx_scene *s) : create(s->svc_mu) {
        for (RayService *v : s->svc) {
            if (!v) continue;
            held.emplace_back(v->mu);
            v->stop_locked();
        }
    }
};

int ensure_state(trx_scene *s) {
    RefitState &r = s->refit;
    if (!r.stream) HIP_TRY(r.stream.create(hipStreamNonBlocking));
    if (!r.result) HIP_TRY(r.result.alloc(1));
    return TRX_OK;
}

// The schedule of the scene's node buffer: derived from one download of the nodes, kept until the entry nodes change.
int ensure_topology(trx_scene *s) {
    RefitState &r = s->refit;
    if (r.have_topology && r.entry_version == s->inst_entry_version) return TRX_OK;
    r.have_topology = false;
    std::vector<CwbvhNode> nodes;
    try {
        nodes.resize(s->n_nodes);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    HIP_TRY(hipMemcpyAsync(nodes.data(), s->nodes.get(), s->n_nodes * TRX_NODE_BYTES, hipMemcpyDeviceToHost, r.stream.get()));
    HIP_TRY(hipStreamSynchronize(r.stream.get()));
    RefitTopology topo;
    const char *why = "";
    const uint32_t *entry = s->h_inst_entry.empty() ? nullptr : s->h_inst_entry.data();
    try {
        const int rc = refit_topology(nodes.data(), s->n_nodes, s->h_inst.empty() ? nullptr : s->h_inst.data(), s->n_inst,
                                      s->tlas_start, entry, topo, &why);
        if (rc) return fail(rc, "refit: %s", why);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    if (!r.order) HIP_TRY(r.order.alloc(s->n_nodes));
    if (!r.seg_base) HIP_TRY(r.seg_base.alloc(s->n_nodes));
    if (!r.boxes) HIP_TRY(r.boxes.alloc(s->n_nodes * 6));
    HIP_TRY(hipMemcpyAsync(r.order.get(), topo.order.data(), s->n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice, r.stream.get()));
    HIP_TRY(hipMemcpyAsync(r.seg_base.get(), topo.seg_base.data(), s->n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice, r.stream.get()));
    HIP_TRY(hipStreamSynchronize(r.stream.get()));
    r.level_start.swap(topo.level_start);
    r.entry_version = s->inst_entry_version;
    r.have_topology = true;
    return TRX_OK;
}

// The refit itself, on `stream`; d_verts (device) holds the new vertices, or h_verts (host) does and is uploaded first.
int scene_refit(trx_scene *s, const float *d_verts, const float *h_verts, uint64_t n_tris, hipStream_t stream, bool own_stream) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    if (!d_verts && !h_verts) return fail(TRX_ERR_INVALID, "null vertex buffer");
    if (s->tri_format != TRX_TRI_VERTS_36 && s->tri_format != TRX_TRI_EDGES_36)
        return fail(TRX_ERR_INVALID, "refit needs a scene created from f32 triangles (tri_format %u)", s->tri_format);
    if (n_tris != s->n_tris) return fail(TRX_ERR_INVALID, "%llu triangles for a scene of %llu", (unsigned long long)n_tris,
                                         (unsigned long long)s->n_tris);
    if (h_verts && !all_finite(h_verts, n_tris * 9)) return fail(TRX_ERR_INVALID, "a vertex coordinate is not finite");
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    if (d_verts && n_tris) {
        // the kernels read d_verts on the scene's device: refuse anything that is not an allocation there, or too short
        hipPointerAttribute_t attr;
        hipDeviceptr_t base = nullptr;
        size_t bytes = 0;
        const bool known = hipPointerGetAttributes(&attr, d_verts) == hipSuccess;
        const bool ranged = known && hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)d_verts) == hipSuccess;
        if (!known || !ranged) (void)hipGetLastError(); // (the query's error is the caller's, not a sticky one)
        if (!known || (attr.type != hipMemoryTypeDevice && !attr.isManaged) || attr.device != s->device)
            return fail(TRX_ERR_INVALID, "d_tri_verts is not device memory of the scene's device %d", s->device);
        if (!ranged || (const char *)d_verts + n_tris * 36 > (const char *)base + bytes)
            return fail(TRX_ERR_INVALID, "d_tri_verts does not hold %llu x 9 floats", (unsigned long long)n_tris);
    }
    int rc = ensure_state(s);
    if (rc) return rc;
    RefitState &r = s->refit;
    if (own_stream) stream = r.stream.get();
    ServicesHeld services(s);
    rc = ensure_topology(s);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    // launches enqueued before this call (any stream) finish on the old geometry before anything is overwritten
    for (Slot &sl : s->slots)
        if (sl.used && sl.done) HIP_TRY(hipStreamWaitEvent(stream, sl.done.get(), 0));
    StreamBuf<float> staged;
    auto release = [&](int code) {
        (void)staged.reset();
        (void)hipStreamSynchronize(stream);
        return code;
    };
    if (h_verts) {
        HIP_TRY(staged.alloc(std::max<uint64_t>(n_tris, 1) * 9, stream));
        if (n_tris && hipMemcpyAsync(staged.get(), h_verts, n_tris * 36, hipMemcpyHostToDevice, stream) != hipSuccess)
            return release(fail(TRX_ERR_NO_DEVICE, "upload of the vertices failed"));
        d_verts = staged.get();
    }
    RefitResult res = {0u, 1u, 1u, 0u};
    if (hipMemcpyAsync(r.result.get(), &res, sizeof(res), hipMemcpyHostToDevice, stream) != hipSuccess)
        return release(fail(TRX_ERR_NO_DEVICE, "refit: upload failed"));
    if (!h_verts) { // (host input was checked above) nothing is written before the check has answered
        if (!refit_launch_check(d_verts, n_tris, r.result.get(), stream) ||
            hipMemcpyAsync(&res, r.result.get(), sizeof(res), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return release(fail(TRX_ERR_NO_DEVICE, "refit: the finiteness check failed to run"));
        if (res.bad_input) return release(fail(TRX_ERR_INVALID, "a vertex coordinate is not finite"));
    }
    const bool xf = s->tlas && !s->inst_o2w.empty();
    if (xf) {
        if (r.o2w.grow((uint64_t)s->n_inst * 16) != hipSuccess) return release(fail(TRX_ERR_OOM, "refit: allocation failed"));
        if (hipMemcpyAsync(r.o2w.get(), s->inst_o2w.data(), (size_t)s->n_inst * 64, hipMemcpyHostToDevice, stream) != hipSuccess)
            return release(fail(TRX_ERR_NO_DEVICE, "refit: upload failed"));
    }
    s->emitters_stale = true; // (the emitter table holds the old triangles in world space: a host flag, no launch changes)
    bool ok = refit_launch_tris(d_verts, n_tris, s->tris.get(), stream);
    RefitCtx ctx;
    ctx.nodes = s->nodes.get();
    ctx.boxes = r.boxes.get();
    ctx.verts = d_verts;
    ctx.seg_base = r.seg_base.get();
    ctx.inst = s->tlas ? s->inst.get() : nullptr;
    ctx.entry = s->tlas ? s->inst_entry.get() : nullptr;
    ctx.o2w = xf ? r.o2w.get() : nullptr;
    ctx.n_inst = s->n_inst;
    ctx.tlas_start = s->tlas_start;
    for (size_t l = 0; ok && l + 1 < r.level_start.size(); l++)
        ok = refit_launch_level(ctx, r.order.get(), r.level_start[l], r.level_start[l + 1] - r.level_start[l], stream);
    ok = ok && refit_launch_stats(s->nodes.get(), s->n_nodes, s->tlas ? s->tlas_start : 0u, r.result.get(), stream);
    ok = ok && hipMemcpyAsync(&res, r.result.get(), sizeof(res), hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = ok && staged.reset() == hipSuccess;
    ok = ok && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return release(fail(TRX_ERR_NO_DEVICE, "refit: a launch failed: %s", hipGetErrorString(hipGetLastError())));
    // the traversal's shortcut flags and the scene scale, derived from the new nodes as trx_scene_create derives them
    s->exp_exact = res.e_ok ? (res.p_ok ? 2u : 1u) : 0u;
    double d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double ext = 255.0 * std::ldexp(1.0, (int)((res.root_e >> (8 * k)) & 0xffu) - 127);
        d2 += ext * ext;
    }
    s->scene_diag = (float)std::sqrt(d2);
    forget_tile_orders(s);
    return TRX_OK;
}

} // namespace

extern "C" {

int trx_scene_refit(trx_scene *scene, const float *tri_verts, uint64_t n_tris) {
    if (!tri_verts) return fail(TRX_ERR_INVALID, "null vertex buffer");
    return scene_refit(scene, nullptr, tri_verts, n_tris, nullptr, true);
}

int trx_scene_refit_dev(trx_scene *scene, const float *d_tri_verts, uint64_t n_tris, void *stream) {
    if (!d_tri_verts) return fail(TRX_ERR_INVALID, "null vertex buffer");
    return scene_refit(scene, d_tri_verts, nullptr, n_tris, (hipStream_t)stream, false);
}

int trx_scene_read_nodes(trx_scene *s, void *out_nodes, uint64_t n_nodes) {
    if (!s || !out_nodes) return fail(TRX_ERR_INVALID, "null argument");
    if (n_nodes != s->n_nodes) return fail(TRX_ERR_INVALID, "%llu nodes for a scene of %llu", (unsigned long long)n_nodes,
                                           (unsigned long long)s->n_nodes);
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu); // (a refit writes the nodes under it)
    HIP_TRY(hipSetDevice(s->device));
    // a stream of its own for the read-back: the null stream would wait for the scene's resident ray services
    Stream stream;
    HIP_TRY(stream.create(hipStreamNonBlocking));
    hipError_t e = hipMemcpyAsync(out_nodes, s->nodes.get(), n_nodes * TRX_NODE_BYTES, hipMemcpyDeviceToHost, stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(stream.get());
    if (e != hipSuccess) return fail(TRX_ERR_NO_DEVICE, "read-back of the nodes failed: %s", hipGetErrorString(e));
    return TRX_OK;
}

int trx_debug_scene_info(trx_scene *s, uint32_t *out_exp_exact, float *out_scene_diag, uint32_t *out_refit_levels) {
    if (!s) return fail(TRX_ERR_INVALID, "null scene");
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    if (out_exp_exact) *out_exp_exact = s->exp_exact;
    if (out_scene_diag) *out_scene_diag = s->scene_diag;
    if (out_refit_levels)
        *out_refit_levels = s->refit.have_topology ? (uint32_t)s->refit.level_start.size() - 1u : 0u;
    return TRX_OK;
}

int trx_refit_nodes(const void *nodes, uint64_t n_nodes, const float *tri_verts, uint64_t n_tris,
                    const uint32_t *instance_offsets, uint32_t n_instances, uint32_t tlas_start, const uint32_t *entry_nodes,
                    const float *object_to_world, void *out_nodes) {
    if (!nodes || !out_nodes || n_nodes == 0) return fail(TRX_ERR_INVALID, "null or empty node buffer");
    if (!tri_verts) return fail(TRX_ERR_INVALID, "null vertex buffer");
    if (n_nodes >= 0xffffffffull || n_tris >= 0xffffffffull) return fail(TRX_ERR_INVALID, "buffer too large for u32 indices");
    if (n_instances && !instance_offsets) return fail(TRX_ERR_INVALID, "instance_offsets is null");
    if (!n_instances && (tlas_start != 0 || entry_nodes || object_to_world))
        return fail(TRX_ERR_INVALID, "tlas_start / entry nodes / transforms without instances");
    int rc = validate_nodes((const CwbvhNode *)nodes, n_nodes, n_tris, instance_offsets, n_instances, tlas_start);
    if (rc == TRX_ERR_FORMAT && !validate_nodes((const CwbvhNode *)nodes, n_nodes, 0xffffffffull, instance_offsets, n_instances, tlas_start))
        return fail(TRX_ERR_INVALID, "the nodes reference more than the %llu triangles given", (unsigned long long)n_tris);
    if (rc) return rc;
    if (entry_nodes && (rc = validate_entries(instance_offsets, n_instances, tlas_start, entry_nodes))) return rc;
    if (!all_finite(tri_verts, n_tris * 9)) return fail(TRX_ERR_INVALID, "a vertex coordinate is not finite");
    if (object_to_world && !all_finite(object_to_world, (uint64_t)n_instances * 16))
        return fail(TRX_ERR_INVALID, "a transform is not finite");
    try {
        RefitTopology topo;
        const char *why = "";
        rc = refit_topology((const CwbvhNode *)nodes, n_nodes, instance_offsets, n_instances, tlas_start, entry_nodes, topo, &why);
        if (rc) return fail(rc, "refit: %s", why);
        std::vector<float> boxes(n_nodes * 6);
        std::memmove(out_nodes, nodes, n_nodes * TRX_NODE_BYTES);
        RefitCtx ctx;
        ctx.nodes = (uint4 *)out_nodes;
        ctx.boxes = boxes.data();
        ctx.verts = tri_verts;
        ctx.seg_base = topo.seg_base.data();
        ctx.inst = n_instances ? instance_offsets : nullptr;
        ctx.entry = entry_nodes;
        ctx.o2w = object_to_world;
        ctx.n_inst = n_instances;
        ctx.tlas_start = tlas_start;
        for (uint32_t i : topo.order) refit_node(ctx, i);
    } catch (const std::exception &) {
        return fail(TRX_ERR_OOM, "host allocation failed");
    }
    return TRX_OK;
}

} // extern "C"
