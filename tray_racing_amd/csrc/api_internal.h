// api_internal.h - what the translation units behind include/trx.h share: the scene object, its launch slots, the
// ray service, error reporting and the launch path (api_launch.cpp).  Not installed; not part of the ABI.
//   api.cpp          errors, devices, scene upload and its setters, the camera
//   api_launch.cpp   enqueue(): launch slots, kernel parameters, tile-order state, the schedule tuner's host side
//   api_trace.cpp    the trace / count / bench / diagnostic entry points (device-resident and host-buffer forms)
//   api_traverse.cpp Traversable::traverse for one ray (the resident ray service) and for batches
//   api_build.cpp    builders, flat-buffer assembly (cwbvh_gpu_runner's host half), scene generators and loaders
//   api_refit.cpp    trx_scene_refit / trx_refit_nodes: the BVH refit's host twin and its device driver (refit_gpu.cpp)
//   api_attr.cpp     trx_hit_attributes_* / trx_trace_rays_attr: the hit-attribute post-pass (k_hit_attr, kernels.hip)
//   api_ao.cpp       trx_ao_rays_dev / trx_trace_ao_visibility*: AO rays as explicit rays, any-hit walk, per-pixel counts;
//                    trx_light_rays_dev / trx_trace_light_visibility_dev / trx_light_term_dev: the same chain per light, and the light term
//                    trx_bounce_light_rays_dev / trx_trace_indirect_dev / trx_trace_indirect_sparse_dev: one diffuse bounce (dense, or over a low grid) - closest-hit bounce rays, their attributes, shadow rays from the bounce hits
//   api_image.cpp    trx_ao_filter_dev / trx_ao_upsample_dev / trx_value_filter_dev / trx_value_upsample_dev / trx_shade_*_dev / trx_render_image* / trx_render_heat_image: the image passes after the walk (image.hip)
//   materials        (include/trx.h, "materials") trx_scene_set_materials / _get_materials in api.cpp; trx_trace_indirect_rgb_dev / _rgb_sparse_dev: the indirect pass's colour mode in api_ao.cpp;
//                    trx_material_compose_dev / trx_shade_rgb_dev / trx_render_image_colour in api_image.cpp; trx_standin_materials / trx_load_model_materials in api_build.cpp (the OBJ/MTL reading itself in scenes.cpp)
//   emitters         (include/trx.h, "emitters") trx_scene_build_emitters / _get_emitters / trx_debug_emitter_select in api_emitters.cpp; trx_emitter_rays_dev / trx_trace_emitter_light_dev and the
//                    indirect pass's emitter mode (trx_trace_indirect_rgb_emitters_dev / _sparse_dev) in api_ao.cpp; trx_render_image_colour_emitters in api_image.cpp
//   vertex normals   (include/trx.h, "vertex normals") trx_scene_set_vertex_normals / _get_vertex_normals in api.cpp; trx_shading_normals_primary_dev / _rays_dev (k_shading_normal, kernels.hip) in api_attr.cpp;
//                    trx_render_image_lit_smooth / _colour_smooth in api_image.cpp; trx_compute_vertex_normals / trx_load_model_normals in api_build.cpp (the welding and the OBJ `vn` reading in scenes.cpp)
//   textures         (include/trx.h, "texture coordinates and albedo textures") trx_scene_set_texcoords / _get_texcoords / trx_scene_set_textures / _get_textures / _remove_textures /
//                    trx_texture_srgb_table in api.cpp; trx_surface_albedo_dev / trx_albedo_compose_dev (k_surface_albedo, k_albedo_compose, image.hip; the sampling rule in texture_dev.h)
//                    in api_image.cpp; trx_standin_texcoords / trx_standin_textures / trx_load_model_texcoords / trx_load_model_material_maps in api_build.cpp (the OBJ `vt` and
//                    mtl `map_Kd` reading in scenes.cpp); image files are decoded in cli.cpp alone (--textures)
//   probe.cpp        trx_debug_fetch_rate: the measured ceiling of the node-fetch loop on a scene's buffers
#ifndef TRX_API_INTERNAL_H
#define TRX_API_INTERNAL_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/trx.h"
#include "../../include/trx_dev.h"
#include "builder.h"
#include "cwbvh_format.h"
#include "hip_owned.h"
#include "image.h"
#include "kernels.h"
#include "scenes.h"

namespace trx {
struct RefitResult; // refit_gpu.h
}
using namespace trx;

namespace trxapi {

// thread-local error string of trx_last_error(); returns `code`
int fail(int code, const char *fmt, ...);
std::string &err_string(); // this thread's error string itself (a launch made for one thread reports to another: api_traverse.cpp)
extern std::atomic<uint32_t> g_variant; // tuning aid (trx_set_kernel_variant), read once per launch

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(e_ == hipErrorOutOfMemory ? TRX_ERR_OOM : TRX_ERR_NO_DEVICE,       \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                    \
    } while (0)

constexpr int kSlots = 8;
constexpr uint32_t kDefaultWavesPerBlock = 1;

struct Slot {
    DevBuf<SlotCounters> ctr;
    DevBuf<uint2> spill; // stack spill area: kWaveScratch entries per wave
    Event done;          // everything enqueued for this slot has finished
    DevBuf<trx_ray> ao_rays;   // trx_trace_ao_visibility_dev on this slot's stream: the rays of one chunk of tiles and samples ...
    DevBuf<uint8_t> ao_flags;  // ... and their occlusion flags (api_ao.cpp)
    // trx_trace_indirect_dev on this slot's stream: per (tile, sample, pixel) of a chunk the bounce ray, its hit, instance id
    // and attribute record and the sample's sum s; per pixel of the chunk's tiles the running sum A (api_ao.cpp)
    DevBuf<trx_ray> gi_rays;
    DevBuf<trx_hit> gi_hits;
    DevBuf<uint32_t> gi_inst;
    DevBuf<trx_hit_attr> gi_attr;
    DevBuf<float> gi_sum, gi_acc;
    // the emitter passes on this slot's stream (api_emitters.cpp; the indirect pass's emitter mode in api_ao.cpp): per
    // (tile, sample, pixel) of a chunk the sample's geometric weight and its emitter; per pixel of the chunk's tiles the
    // primary pass's three running sums
    DevBuf<float> em_wgeo, em_acc;
    DevBuf<uint32_t> em_pick;
    // trx_value_filter_dev on this slot's stream with d_base == d_out and three levels or more: the second intermediate plane,
    // which cannot sit in d_out then (api_image.cpp)
    DevBuf<float> vf_plane;
    bool used = false;
    bool pinned = false;               // a resident kernel (the ray service) runs on this slot: never recycled for another stream
    hipStream_t last_stream = nullptr; // stream of the last launch on this slot
    uint64_t last_use = 0;             // launch counter at that time (oldest slot is recycled first)
    bool ray_cost_set = false;         // ctr->ray_cost may be non-null: the next counting launch on the slot rewrites it
    // tile-cost feedback: the previous frame of a kind (primary / AO) traced on this slot measured every tile; the
    // next one of that kind with the same image geometry starts its heaviest tiles first.  One state per kind: the
    // reference's frame loop runs both passes on one queue, and each has its own order.
    struct Order {
        DevBuf<uint32_t> lists; // two sets of {128 counts, 128 lists}: 16 cost buckets x kLptShards shards (api_launch.cpp)
        uint32_t capacity = 0;  // tiles the lists are sized for
        bool have_views = false; // view[] holds the views of a previous launch
        uint64_t key = 0;    // (width, height, shard, mode) the lists were measured for; 0 = none
        ViewDev view[kMaxBatchFrames]{}; // views of the last launch that read or wrote the lists (camera-cut detection)
    } order[2];
};

// trx_scene_refit's per-scene state (api_refit.cpp; the stream and result word are created on first use)
struct RefitState {
    Stream stream;                    // read-backs and the host-memory refit
    bool have_topology = false;
    uint64_t entry_version = 0;       // s->inst_entry_version the schedule was derived for
    std::vector<uint32_t> level_start;
    DevBuf<uint32_t> order, seg_base;
    DevBuf<float> boxes;
    DevBuf<float> o2w;                // the instances' object-to-world matrices (16 floats each)
    DevBuf<RefitResult> result;
};

} // namespace trxapi

// trx_frame_loop's streams, events and device buffers (created on first use)
struct FrameLoop {
    static constexpr int kBuffers = 4; // primary-hit buffers: the primary passes may run this many frames ahead of the AO passes
    trxapi::Stream stream[2];
    trxapi::Event prim_done[kBuffers], ao_done[kBuffers], t0, t1;
    trxapi::DevBuf<trx_hit> prim[kBuffers], ao;
    trxapi::DevBuf<uint32_t> prim_inst[kBuffers], ao_inst;
    uint64_t records = 0; // every buffer holds this many records
};

// trx_traverse1: a RESIDENT kernel answers the callers' rays out of a ring in pinned host memory
// (kernels.h, kSvcRays; kernel side in trace_service.inc) - no launch, no stream synchronisation per ray.  A caller claims
// a slot, writes its ray as three 16-byte granules that carry a fresh sequence number, and spins on the slot's answer
// word.  The kernel is started by the first call and stopped by a watchdog thread after kIdleStopNs without a call (or by
// trx_scene_destroy), so that device-wide synchronisations elsewhere in the process wait for it no longer than that; the
// same thread bumps the heartbeat without which the kernel leaves by itself.
struct RayService {
    static constexpr uint32_t kGroups = 16, kSlots = kGroups * trx::kSvcRays;
    static constexpr int64_t kIdleStopNs = 50 * 1000 * 1000, kBeatNs = 2 * 1000 * 1000, kGiveUpNs = 5LL * 1000 * 1000 * 1000;
    trx_scene *scene = nullptr;
    uint32_t sem = 0;
    trxapi::HostBuf<uint32_t> ring, ctl; // pinned, device-visible
    trxapi::Stream stream;
    std::mutex mu;                    // start / stop
    std::atomic<bool> running{false};
    // Per slot, on cache lines of its own: everything a call writes on the host side.  (Until late in round 6 every call
    // bumped seven process-wide words - a count of callers inside, the last use, four statistics - and the slots' busy
    // flags sat sixteen to a line: from ten threads on the calls queued for those lines, 2.2-2.5 us apiece system-wide,
    // whatever the walk took - 0.40-0.47 Mrays/s was that queue, not the GPU.)
    struct alignas(128) Caller {
        std::atomic<uint32_t> busy{0};     // a caller owns the slot
        uint32_t seq = 0;                  // last sequence number used on the slot (its current owner's to bump)
        std::atomic<int64_t> last_use_ns{0};
        std::atomic<uint64_t> rays{0}, walk_ticks{0}, walk_trips{0}, call_ns{0}; // statistics (trx_debug_service_stats)
    };
    Caller caller[kSlots];
    std::thread watchdog;
    std::atomic<bool> quit{false};
    bool ok = false;
    std::string init_err;
    std::atomic<uint64_t> starts{0};
    bool idle_since(int64_t t_ns) const { // no slot owned, none used since t_ns
        for (const Caller &c : caller)
            if (c.busy.load(std::memory_order_acquire) != 0u || c.last_use_ns.load(std::memory_order_relaxed) > t_ns) return false;
        return true;
    }
    uint64_t sum(std::atomic<uint64_t> Caller::*field) const {
        uint64_t n = 0;
        for (const Caller &c : caller) n += (c.*field).load(std::memory_order_relaxed);
        return n;
    }
    RayService(trx_scene *s, uint32_t semantics);
    ~RayService();
    int start_locked();  // mu held
    void stop_locked();  // mu held
};

struct trx_scene {
    int device = 0;
    trxapi::DevBuf<uint4> nodes;
    trxapi::DevBuf<float4> tris;
    trxapi::DevBuf<uint32_t> inst;
    trxapi::DevBuf<uint32_t> inst_entry;     // entry node per TLAS primitive (re-braided scenes), or empty
    std::vector<uint32_t> h_inst;            // host copy of the instance offsets (entry-node validation)
    uint64_t n_nodes = 0, n_tris = 0;
    uint32_t n_inst = 0, tlas_start = 0;
    bool tlas = false;
    float scene_diag = 0.f; // diagonal of the root node's box (camera-cut detection scales with it)
    uint32_t exp_exact = 0u; // 1: every node exponent byte is 0 or >= 21; 2: and every node origin admits div_by_rcp (TraceParams::exp_exact)
    int grid = 0;      // default number of persistent waves
    int cu_count = 0;
    trxapi::DevBuf<unsigned long long> wave_times; // diagnostics only (trx_debug_wave_timeline)
    uint32_t *dbg_cost = nullptr, *dbg_iters = nullptr; // diagnostics only: trx_debug_tile_profile's buffers while it runs
    trx_ray_cost *count_cost = nullptr; // trx_count_*_per_ray's record buffer while the call runs (under host_mu), else null
    trxapi::Slot slots[trxapi::kSlots];
    uint64_t launches = 0;
    std::mutex mu;      // launch slots (every enqueue)
    std::recursive_mutex host_mu; // scratch buffers and event pair of the synchronous entry points
    // scratch for the host-buffer convenience entry points
    trxapi::DevBuf<trx_hit> scratch_a, scratch_b;
    trxapi::DevBuf<uint32_t> scratch_ia, scratch_ib; // instance ids beside scratch_a / scratch_b (two-level scenes)
    trxapi::DevBuf<trx_ray> scratch_rays;
    trxapi::DevBuf<trx_hit_attr> scratch_attr; // trx_trace_rays_attr's attribute records (api_attr.cpp)
    trxapi::Event ev0, ev1;
    std::vector<uint32_t> blas_tri_start; // geometry_id lookup for trx_traverse1
    FrameLoop loop;                // trx_frame_loop
    RayService *svc[8] = {};       // trx_traverse1: one resident kernel per semantics word in use
    std::mutex svc_mu;             // creation of the services
    // instance transforms (TLAS scenes): object-to-world as given (get_instance_transform), world-to-object rows as
    // the kernels use them, and their device copy; empty / null = identity
    std::vector<float> inst_o2w, inst_w2o;
    trxapi::DevBuf<float4> inst_xform;
    uint32_t tri_format = 0;                 // trx_tri_format the scene was created from (trx_scene_refit takes the f32 ones)
    std::vector<uint32_t> h_inst_entry;      // host copy of the entry nodes (empty = node 0 everywhere) ...
    uint64_t inst_entry_version = 0;         // ... bumped whenever they are set: the refit's cached schedule follows them
    trxapi::RefitState refit;                // trx_scene_refit: schedule, node boxes, stream (api_refit.cpp)
    // instance masks (TLAS scenes, trx_scene_set_instance_masks): one byte per TLAS primitive, read by the masked trace
    // calls only; host copy and device table, empty = every instance 0xFF
    std::vector<uint8_t> h_inst_mask;
    trxapi::DevBuf<uint8_t> inst_mask;
    // materials (trx_scene_set_materials): the table and one index per triangle in `prim` order, every index validated
    // against the table on upload; host copies and device tables, swapped together under mu; empty = no materials (the
    // colour entry points are refused)
    std::vector<trx_material> h_materials;
    std::vector<uint16_t> h_tri_material;
    trxapi::DevBuf<trx_material> materials;
    trxapi::DevBuf<uint16_t> tri_material;
    // emitters (trx_scene_build_emitters, api_emitters.cpp): the world-space records (four float4 each) and the n - 1
    // cumulative selection probabilities, host copies and device tables, swapped together under mu; stale once the
    // materials, the triangles or the instances changed under them (every emitter entry point then refuses)
    std::vector<float> h_emitters, h_emitter_cdf;
    trxapi::DevBuf<float4> emitters;
    trxapi::DevBuf<float> emitter_cdf;
    uint32_t n_emitters = 0;
    bool emitters_stale = false;
    // the frame's image (api_image.cpp): the shade's 256 code thresholds on the scene's device (first shade; under mu), and
    // trx_render_image's scratch - the filter's terms, then the RGBA8 image (under host_mu)
    trxapi::DevBuf<float> image_thr;
    trxapi::DevBuf<uint8_t> scratch_img;
    // vertex normals (trx_scene_set_vertex_normals): the caller's nine floats per triangle in `prim` order and the device
    // table of three float4 per triangle (w = +0), swapped together under mu; empty = no table (the shading-normal entry
    // points are refused)
    std::vector<float> h_vertex_normals;
    trxapi::DevBuf<float4> vertex_normals;
    // texture coordinates (trx_scene_set_texcoords): the caller's six floats per triangle in `prim` order and the device
    // table of three float2 per triangle, swapped together under mu; empty = no table (the albedo pass writes the plain albedo)
    std::vector<float> h_texcoords;
    trxapi::DevBuf<float2> texcoords;
    // the texture set (trx_scene_set_textures): descriptors, texel words and the per-material texture index as the caller
    // gave them, and on the device {offset, width, height, format | filter << 8} per texture, the texels, the index and the
    // sRGB decode table; every index validated on upload, all swapped together under mu; empty = no set
    std::vector<trx_texture_desc> h_tex_descs;
    std::vector<uint32_t> h_texels, h_material_texture;
    trxapi::DevBuf<uint4> tex_descs;
    trxapi::DevBuf<uint32_t> texels, material_texture;
    trxapi::DevBuf<float> tex_srgb;
};

struct trx_bvh {
    CwBvh bvh;
};

namespace trxapi {

// the host-buffer entry points' scratch: at least `hits` records (and instance ids on two-level scenes), `rays` rays and
// `attrs` attribute records
int ensure_scratch(trx_scene *s, uint64_t hits, uint64_t rays, uint64_t attrs = 0);
void fill_view(const trx_view *v, trx::ViewDev &out);
// The launch slot a kernel enqueued on `stream` runs on, set up and waited for (api_launch.cpp; s->mu held)
int acquire_slot(trx_scene *s, hipStream_t stream, Slot *&out);
// Enqueues one traversal kernel on a launch slot of the scene (api_launch.cpp)
int enqueue(trx_scene *s, trx::TraceParams &p, int mode, uint32_t sem, bool count, hipStream_t stream, trx::SlotCounters **ctr_out);
// ... the same for a caller that holds s->mu and has set the device and checked `sem` (a pass of several launches on one slot)
int enqueue_locked(trx_scene *s, trx::TraceParams &p, int mode, uint32_t sem, bool count, hipStream_t stream, trx::SlotCounters **ctr_out);
// an image pass's kernel parameters: p zeroed, then the geometry of `view` / w x h / shard
// whether a launch of `mode` on the scene takes the pipelined walk (api_launch.cpp); the shipped decision, no tuning bits
bool pipelined_walk(const trx_scene *s, int mode);
int image_params(trx::TraceParams &p, const trx_view *view, uint32_t w, uint32_t h, trx_shard shard);
int read_overflow(trx_scene *s, trx::SlotCounters *ctr);
// structural validation of an untrusted node buffer (api.cpp): every index a walk can form is in range
int validate_nodes(const CwbvhNode *nodes, uint64_t n_nodes, uint64_t n_tris, const uint32_t *inst, uint32_t n_inst,
                   uint32_t tlas_start);
// the scene under the launch slots' learnt tile orders changed: the next frame of every slot files a new order (s->mu held)
void forget_tile_orders(trx_scene *s);
// device bytes of trx_scene_refit's per-scene state (api_refit.cpp)
uint64_t refit_state_bytes(const trx_scene *s);
// explicit rays (api_trace.cpp)
// (ray_mask != 0: a masked trace - enqueue() hands the kernel the scene's instance mask table)
int trace_rays_impl(trx_scene *s, const trx_ray *d_rays, uint64_t n, uint32_t sem, trx_hit *d_hits, hipStream_t stream, bool count,
                    trx::SlotCounters **ctr, bool any_hit = false, uint32_t *d_inst = nullptr, uint32_t ray_mask = 0);

// what the direct-light entry points refuse of their lights and sample count (api_ao.cpp)
int check_lights(const trx_light *lights, uint32_t n_lights, uint32_t n_samples);

// what every emitter entry point refuses of the scene's emitter table (api_emitters.cpp; s->mu held) and of emitter_eps
int need_emitters(const trx_scene *s);
int check_emitter_eps(float emitter_eps);

// ---- the synchronous host-buffer entry points (api_trace.cpp, api_attr.cpp) ----
// ev0, what `run` enqueues on the null stream, ev1; waits for ev1 and puts the elapsed time into *ms (may be null)
template <typename Run>
int timed(trx_scene *s, float *ms, Run run) {
    HIP_TRY(hipEventRecord(s->ev0.get(), nullptr));
    if (int rc = run()) return rc;
    HIP_TRY(hipEventRecord(s->ev1.get(), nullptr));
    HIP_TRY(hipEventSynchronize(s->ev1.get()));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, s->ev0.get(), s->ev1.get()));
    return TRX_OK;
}
// One host-buffer call: under host_mu (the scratch and the event pair are shared) on the scene's device, scratch for
// `hits` records and `attrs` attribute records, the n_rays `rays` uploaded when given, `run` timed, then `read` copies
// the results back and trx_scene_check reports an overflow.
template <typename Run, typename Read>
int host_call(trx_scene *s, uint64_t hits, const trx_ray *rays, uint64_t n_rays, uint64_t attrs, float *out_ms, Run run, Read read) {
    std::lock_guard<std::recursive_mutex> host_lock(s->host_mu);
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = ensure_scratch(s, hits, rays ? n_rays : 0, attrs)) return rc;
    if (rays) HIP_TRY(hipMemcpy(s->scratch_rays.get(), rays, n_rays * sizeof(trx_ray), hipMemcpyHostToDevice));
    if (int rc = timed(s, out_ms, run)) return rc;
    if (int rc = read()) return rc;
    return trx_scene_check(s, nullptr);
}
// n instance ids back into dst (may be null): the device's, or 0xFFFFFFFF everywhere on a scene without a TLAS (src null)
int read_inst(uint32_t *dst, const uint32_t *src, uint64_t n);

} // namespace trxapi

using namespace trxapi;

#endif // TRX_API_INTERNAL_H
