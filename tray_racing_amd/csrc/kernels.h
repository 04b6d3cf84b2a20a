// kernels.h — launch interface between the C-ABI layer (api_launch.cpp) and the
// gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/trx.h"
#include "texture_dev.h"

namespace trx {

constexpr int kWave = 64;          // gfx950 wavefront
constexpr int kMaxBlock = 256;     // up to 4 waves per workgroup
constexpr uint32_t kLptShards = 8; // appenders per tile-cost bucket (16 buckets x 8 shards = 128 lists)
#ifndef TRX_LDS_STACK
#define TRX_LDS_STACK 12
#endif
#ifndef TRX_MIN_WAVES
#define TRX_MIN_WAVES 4 // waves per SIMD the register allocator must leave room for
#endif
#ifndef TRX_TRI_BATCH
#define TRX_TRI_BATCH 1
#endif
#ifndef TRX_TRI_BATCH_TLAS
#define TRX_TRI_BATCH_TLAS 1
#endif
#ifndef TRX_TRI_BATCH_PIPE
#define TRX_TRI_BATCH_PIPE 1
#endif
// triangles of a lane requested together in a per-lane triangle round: BLAS-only walk / two-level walk / pipelined walk
constexpr int kTriBatch = TRX_TRI_BATCH, kTriBatchTlas = TRX_TRI_BATCH_TLAS, kTriBatchPipe = TRX_TRI_BATCH_PIPE;
constexpr int kLdsStack = TRX_LDS_STACK;        // traversal-stack entries per lane kept in LDS
constexpr int kSpillStack = 64 - TRX_LDS_STACK; // further entries per lane in HBM (total 64 = oracle's ORC_STACK_SIZE)
// A wave's private HBM area (TraceParams::spill, in uint2 entries): the stack entries past the LDS part, then the WORLD-SPACE
// rays of its lanes ([6][64] floats: origin, direction as given) - a two-level walk over instance transforms comes back
// to them when it leaves a BLAS, and six registers that are read on that path only are six registers the walk does not have
constexpr int kWaveScratch = kSpillStack * kWave + 3 * kWave;
// LDS per wave: stack + ray table (2 x float4 per lane) + triangle-phase tables (group, result, prefix, heads)
constexpr int kLptPend = 32; // tile-list appends a wave parks in LDS before issuing them together
constexpr int kLdsBytesPerWave = TRX_LDS_STACK * kWave * 8 + kWave * 32 + kWave * 8 + kWave * 8 + kWave * 4 + kWave * 4 + kLptPend * 8 + 6 * 8 * 4 + 64; // ... + the decoded child planes of a wave-uniform node step + the packet test's ray bounds (16 waves per CU = 160 KB exactly)
constexpr int kWaveTimeStride = 8; // diagnostics record per wave: start, end, then (TRX_STAMPS builds) phase cycles
constexpr uint32_t kMaxSteps = 1u << 22; // per-ray iteration cap: every wave reaches an exit

// kModeFused: the reference's whole pixel program in one launch (rt_gpu_software.hlsl:47-144): a lane whose primary
// ray ends in a hit becomes that pixel's AO ray in place
// kModeService: a resident kernel that answers single-ray requests out of a ring in pinned host memory (trx_traverse1:
// Traversable::traverse called ray by ray from a thread pool, src/rt_cpu/rt_cpu.rs:35-57) - no launch per ray, see below
enum TraceMode : int { kModePrimary = 0, kModeAo = 1, kModeRays = 2, kModeFused = 3, kModeService = 4 };

// The ray service (k_trace<kModeService>; api_traverse.cpp holds the host side).  A workgroup is two waves: the WALKER
// steps up to kSvcRays rays, eight lanes to a ray (the thin walk of an incoherent pass's last rays), and reads nothing
// from host memory - a load from it takes 1.5-2 us, and a wave's loads return in order, so a poll in flight would hold up
// every node fetch behind it; the PORTER polls the workgroup's kSvcRays request slots - through the SCALAR cache: a CU's
// vector-memory path makes the walker's requests wait for the porter's as well (trace_service.inc) - and hands complete
// requests to the walker through mailboxes in LDS; the walker stores its answers into the slots' answer words itself.
//   slot k of the ring = 128 bytes: [0..47] the request, three 16-byte granules {ox oy oz seq}{dx dy dz seq}{tmin tmax 0
// seq}, each written by ONE 16-byte store of the host (a request is complete when the three carry the same seq, and new
// when that differs from the slot's last answer); [64..79] the answer {t, prim, overflow, seq}, one 16-byte store of the
// GPU.  Host and GPU never write the same 64-byte line.
//   control words (pinned host memory): [0] != 0: leave (set when no caller is inside trx_traverse1); [1] a heartbeat
// the host bumps every few milliseconds while the service is up - a porter that sees it stand still for kSvcDeadTicks of
// the 100 MHz wall clock takes the host for dead and leaves as well: every wave of the grid reaches its exit.
constexpr uint32_t kSvcRays = 4;                 // request slots per workgroup (one ray per eight lanes of the walker's lower half: the porter reads a workgroup's requests in ONE look - 4 x 12 words are what its scalar registers hold)
constexpr uint32_t kSvcSlotWords = 32;           // 128 bytes per slot
constexpr unsigned long long kSvcDeadTicks = 200000000ull; // 2 s without a heartbeat

constexpr int kMaxBatchFrames = 8;

struct ViewDev {
    float view_inv[16];
    float proj_inv[16];
    float eye[3];
    float pad;
};

// Device-side counters of one launch slot.
struct alignas(128) QueueHead {
    unsigned int taken; // chunks handed out from this queue (self-resetting)
    unsigned int pad[31];
};

// Self-tuning of the frame schedule (k_trace exit protocol): start stamp of the running frame; the mode the frames run
// in (0 = whole tiles, heaviest first from the learnt order; 1 = whole tiles in natural order, no feedback machinery;
// 2 = natural order, finished rays replaced once kFbRefill lanes idle); frames run in the current phase; the phase
// (0..2 = measuring that mode, 3 = holding the winner); best frame time (100 MHz ticks) seen per mode.
struct FbState {
    unsigned long long t0;
    unsigned int mode, frames, phase, t[3];
};

struct SlotCounters {
    QueueHead heads[8];      // one work-queue head per XCD, each on its own 128-byte line
    unsigned int waves_done; // exit ticket (self-resetting)
    unsigned int overflow;   // rays whose stack overflowed or that hit the step cap (sticky)
    unsigned int pad;
    unsigned long long n_rays, n_node, n_tri, n_hits; // COUNT kernels only
    unsigned int max_stack;
    unsigned int pad2;
    unsigned long long n_wave_node, n_wave_tri; // wave-level node / triangle step executions
    // COUNT kernels: per triangle phase, histogram of the largest per-lane triangle count (0..15+) and of the
    // wave's pair total in units of 8 (0..15+)
    unsigned int hist_max[16], hist_total[16];
    // self-tuning of the frame schedule, one state per pass kind (0 = primary, 1 = AO: a frame loop runs both on one stream)
    FbState fb[2];
    unsigned int lpt_sel[2]; // which of a kind's two tile-list sets holds the order to read (TraceParams::lpt_sel)
    // COUNT kernels only (trx_count_*_per_ray): one trx_ray_cost per record, indexed like the pass's hit buffer, or null.  It
    // travels here and not in TraceParams, which has no eight bytes to spare (its size is fixed, below) and no field that a
    // timed kernel does not read; enqueue_locked writes it ahead of a counting launch that has such a buffer, finish_count
    // clears it.
    trx_ray_cost *ray_cost;
};

struct TraceParams {
    const uint4 *nodes;
    const float4 *tris;
    const uint32_t *inst;
    const uint32_t *inst_entry; // node of its BLAS at which a TLAS primitive's walk starts (null: node 0, the reference's rule)
    const trx_ray *rays;
    const trx_hit *primary;
    trx_hit *out;
    trx_hit *out_ao;        // kModeFused: the AO pass's records (out = the primary pass's)
    uint32_t *out_ao_inst;  // ... and their instance ids (TLAS scenes), or null
    uint32_t thin_max;      // a dry wave with this many rays or fewer gives every ray several lanes (kernels.hip, thin_walk); 0 = never
    uint32_t pend_min;      // kModeFused, queues dry: convert finished primary rays to AO rays once this many lanes wait
    // instance transforms (TLAS scenes; all null = the reference's identity behaviour): world-to-object rows
    // {m0 m1 m2 t} x 3 per TLAS primitive; the instance each hit was found in, per record like `out`; the
    // primary pass's instance ids (AO mode: to take the hit triangle's normal into world space)
    const float4 *inst_xform;
    uint32_t *out_inst;
    const uint32_t *primary_inst;
    SlotCounters *ctr;
    uint2 *spill;
    uint32_t n_items;
    uint32_t tlas_start;
    uint32_t width, height, tiles_x;
    uint32_t shard_index, shard_count;
    uint32_t compact; // TRX_LAYOUT_SHARD: hit buffers indexed by local_tile*64 + pixel-in-tile
    uint32_t single_queue;  // tuning: one global queue instead of one per XCD
    // tile order feedback: 16 x kLptShards list counts + lists (lpt_cap entries each) read / written this frame
    // Two list sets of lpt_set_words words each ({16 x kLptShards counts}{16 x kLptShards lists of lpt_cap tile ids}) at
    // lpt_sets (null: no feedback); *lpt_sel (0 / 1, device side: the exit wave of a learning frame flips it) names the
    // set this frame reads, the other one is empty and takes what a learning frame files.
    uint32_t *lpt_sets;
    unsigned int *lpt_sel;
    uint32_t lpt_set_words;
    uint32_t lpt_cap;
    uint32_t same_view;     // the views of this launch are those of the previous launch of this kind on the slot: a complete
                            // order is replayed as it is - nothing is timed or filed (a FROZEN order, kernels.hip)
    uint32_t *cost;         // diagnostics: per-tile cost (wall-clock ticks), or null
    uint32_t prio_cut[3];   // chunks below these (heaviest-first) indices run at s_setprio 3 / 2 / 1
    uint8_t *touch_nodes, *touch_tris; // diagnostics (COUNT kernels): byte set per node fetched / triangle tested, or null
    uint32_t *tile_iters;   // diagnostics (COUNT kernels): per tile (node steps << 16) | triangle rounds
    uint32_t frame;
    float ao_eps;
    uint32_t tie_first;
    uint32_t refill_idle; // refill the wave when at least this many lanes are idle (1..64)
    uint32_t tri_compact_min; // consider spreading the wave's triangle tests over all lanes when a lane owns this many
    uint32_t tri_coop_ratio;  // ... and do it when the largest per-lane count exceeds this x the cooperative rounds
    uint32_t variant;
    uint32_t tune;                   // development switches (TRX_TUNE environment word), 0 in the product
    uint32_t n_tris, n_nodes;        // buffer extents (prefetch addresses are clamped to them)
    uint32_t waves_per_block;        // 1, 2 or 4
    uint32_t merge;                  // 2 waves per workgroup, incoherent BLAS pass: the second wave may hand its last rays to the first (kernels.hip, drain)
    unsigned long long *wave_times;  // diagnostics: [8*wave] start, [8*wave+1] end (wall_clock64), [+2..7] phase cycles in TRX_STAMPS builds; or null
    FbState *fb;          // image passes with tile-order feedback: the schedule tuner's state (null = feedback always on)
    uint32_t exp_exact;   // >= 1: every exponent byte of the scene's nodes is 0 or >= 21: e / d may be computed as e * (1/d) exactly; 2: and every node origin is +0 or within 2^-36 .. 2^59: (p - o) / d from 1/d by one correction step (kernels.hip, TRX_NODE_FRAME)
    uint32_t no_order;    // ignore the order on file (this frame files a new one): first frame of an image geometry
    uint32_t new_view;    // camera cut: the schedule tuner starts over
    uint32_t uni_decode;  // coherent primary walk: decode the child planes of a node step once per wave when every lane visits the same node
    uint32_t any_hit;     // explicit rays only: stop at the first accepted hit, write one byte (0/1) per ray
    // kModeService: the request / answer ring and the control words (all pinned host memory), see kSvcRays
    uint32_t *svc_ring;
    const uint32_t *svc_ctl;
    uint32_t *over_host;  // null, or a word in pinned host memory that is set when a ray of THIS launch overflows (no host
                          // caller sets it since round 5's combiner was removed; it goes with the kernel's check in a measured change)
    // frames per launch: primary passes - frame f = local_tile / tiles_per_frame uses views[f]; AO passes - one view
    // (views[0]) and one primary buffer, frame f uses the noise seed frame + f (a tile's seeds are consecutive tickets of
    // one queue); either way frame f writes its records at out + f * frame_stride
    uint32_t n_frames, tiles_per_frame, frame_stride;
    // floor(2^32 / d) of the four launch-uniform divisors the refill divides by (kernels.hip, div_uniform): filled in by
    // enqueue(); left to the compiler each division keeps its reciprocal in a VECTOR register for the whole kernel
    uint32_t rcp_tiles_x, rcp_width, rcp_tiles_per_frame, rcp_n_frames;
    ViewDev views[kMaxBatchFrames];
    uint32_t ray_mask; // instance masks: the masked calls' ray mask (1..255), 0 for every other launch (see TraceParamsTlas)
};
// The two-level kernels' parameters: TraceParams, then the instance mask table of the masked trace calls
// (trx_trace_*_masked*): one byte per TLAS primitive; the two-level walk enters primitive k only if
// (inst_mask[k] & ray_mask) != 0.  Null: every instance is entered (the unmasked calls, and masked calls on a scene without
// a table).  The single-level kernels take TraceParams alone: ray_mask sits in what was its tail padding, so TraceParams
// keeps its 1536 bytes and the single-level kernels' arguments - the hidden ones behind them included - keep their offsets.
// n_inst, the extent of inst_xform, sits here for the same reason: only a two-level AO pass over instance rows reads it.
struct TraceParamsTlas : TraceParams {
    const uint8_t *inst_mask;
    uint32_t n_inst; // rows of inst_xform (the AO refill reads it with them, and only there: instance_row below)
};
static_assert(sizeof(TraceParams) == 1536, "TraceParams grew: every single-level kernel's hidden arguments would move");

// Caller records (include/trx.h, "CALLER RECORDS"): the passes that take primary records from the caller index the scene's
// triangle table with a record's prim and its instance rows with the id beside it.  This is the one statement of which
// records and ids may: a SURFACE record has t < FLT_MAX and prim < n_tris (0xFFFFFFFF is never below it), every other record
// is a miss; an id >= n_inst selects no row.  One unsigned comparison each - no address is formed from a value that fails it.
__host__ __device__ inline bool surface_record(const trx_hit &h, uint32_t n_tris) { return h.t < 3.402823466e+38f && h.prim < n_tris; }
__host__ __device__ inline bool instance_row(uint32_t inst, uint32_t n_inst) { return inst < n_inst; }

// The image geometry of a tile-ordered pass as the small kernels take it: the fields of TraceParams of the same names.
struct TileGeom {
    uint32_t width, height, tiles_x, shard_index, shard_count, compact;
};
inline TileGeom tile_geom(const TraceParams &t) { return TileGeom{t.width, t.height, t.tiles_x, t.shard_index, t.shard_count, t.compact}; }

// Hit attributes (k_hit_attr, trx_hit_attributes_*): one lane per hit record, no traversal.
enum HitAttrMode : int { kAttrRays = 0, kAttrPrimary = 1 };
struct HitAttrParams {
    const float4 *tris;       // the scene's 48-byte records
    const float4 *inst_xform; // world-to-object rows per instance, or null (no instance transforms)
    const trx_ray *rays;      // kAttrRays
    const trx_hit *hits;
    const uint32_t *inst;     // instance id per record (read only with inst_xform)
    trx_hit_attr *out;
    uint32_t n_items;         // kAttrRays: records; kAttrPrimary: the shard's tiles * 64, in tile order
    uint32_t n_tris, n_inst;
    TileGeom geom;            // kAttrPrimary
    ViewDev view;
};
hipError_t launch_hit_attr(const HitAttrParams &p, int mode, hipStream_t stream);

// The shading normal (k_shading_normal, trx_shading_normals_*): one lane per record, indexed exactly as HitAttrParams'
// records are; `normals` holds three float4 per triangle (the vertex normals of vertices 0, 1, 2, w = +0), n_tris of them.
struct ShadingNormalParams {
    const float4 *normals;
    const float4 *inst_xform; // world-to-object rows per instance, or null (no instance transforms)
    const trx_ray *rays;      // kAttrRays (the direction words alone are read)
    const trx_hit *hits;
    const uint32_t *inst;     // instance id per record (read only with inst_xform)
    const trx_hit_attr *attr;
    trx_hit_attr *out;        // may be attr
    uint32_t n_items;         // kAttrRays: records; kAttrPrimary: the shard's tiles * 64, in tile order
    uint32_t n_tris, n_inst;
    TileGeom geom;            // kAttrPrimary
    ViewDev view;
};
hipError_t launch_shading_normal(const ShadingNormalParams &p, int mode, hipStream_t stream);

// AO visibility (trx_ao_rays_dev / trx_trace_ao_visibility_dev): k_ao_rays writes the AO pass's rays as explicit rays, the
// any-hit rays launch walks them, k_ao_reduce adds the flags into per-pixel counts.  One lane per (tile, sample, pixel).
//   record layout (scratch == 0, one sample): rays[record], records laid out by the shard like the hit buffers; pixels
// outside the image are left alone.
//   scratch layout (scratch == 1): rays[((tile - tile0) * n_samples + sample) * 64 + pixel-in-tile] for the shard's local
// tiles tile0 .. tile0 + n_tiles - 1 and the seeds frame .. frame + n_samples - 1; EVERY entry is written (pixels outside the
// image and primary misses get the inert ray), because the rays launch walks all of them.
//   sparse (stride != 0, trx_trace_ao_visibility_sparse_dev; scratch layout, whole image): the tiles are those of the LOW
// grid `lo` (ceil(width / stride) x ceil(height / stride) cells); cell (X, Y) stands for pixel (X * stride + px0,
// Y * stride + py0) of the full image `geom`, whose record and coordinates the ray is built from exactly as in the dense
// pass; a cell whose pixel leaves the image gets the inert ray and the count TRX_AO_NO_SURFACE.  counts holds one byte per
// cell, Y * lo.width + X.  The dense launches leave stride 0 and run the kernels' dense instantiations.
constexpr uint32_t kAoNoSurface = 0xffu;        // TRX_AO_NO_SURFACE
constexpr uint32_t kAoUnitBytes = 64u * 32u + 64u; // scratch per (tile, sample): 64 rays and their 64 flags
struct AoRaysParams {
    const float4 *tris;
    const float4 *inst_xform;     // world-to-object rows per instance, or null (no instance transforms)
    const trx_hit *primary;
    const uint32_t *primary_inst; // read only with inst_xform
    trx_ray *rays;
    const uint8_t *flags;         // k_ao_reduce: the occlusion flags of the scratch rays
    uint8_t *counts;              // k_ao_reduce: one byte per record, laid out by the shard
    uint32_t tile0, n_tiles, n_samples, scratch;
    uint32_t first;               // k_ao_reduce: the first samples of these tiles (counts are set, not added to)
    TileGeom geom;
    uint32_t frame;
    float ao_eps, tmax;
    ViewDev view;
    uint32_t stride, px0, py0;    // sparse: 1..TRX_MAX_AO_STRIDE and the phase's pixel in the stride x stride block (dense: 0)
    TileGeom lo;                  // sparse: the low grid (whole image, image layout)
    uint32_t n_tris, n_inst;      // the extents of tris and inst_xform: what a caller's record may index (surface_record; last: the fields above keep their offsets)
};
hipError_t launch_ao_rays(const AoRaysParams &p, hipStream_t stream);
hipError_t launch_ao_reduce(const AoRaysParams &p, hipStream_t stream);

// Direct light (trx_light_rays_dev / trx_trace_light_visibility_dev / trx_light_term_dev): the AO visibility pass's shape,
// once per light.  k_light_rays writes the shadow rays of ONE light (carried by value) as explicit rays - record layout or
// scratch layout exactly as AoRaysParams describes them, one lane per (tile, sample, pixel); the any-hit rays launch walks
// them; k_light_reduce adds the flags into the light's plane of per-pixel counts (an inert ray counts as not lit; a pixel
// without a surface - its primary record says so - gets TRX_AO_NO_SURFACE).
struct LightRaysParams {
    const float4 *tris;
    const float4 *inst_xform;     // world-to-object rows per instance, or null (no instance transforms)
    const trx_hit *primary;
    const uint32_t *primary_inst; // read only with inst_xform
    trx_ray *rays;
    const uint8_t *flags;         // k_light_reduce: the occlusion flags of the scratch rays
    uint8_t *counts;              // k_light_reduce: the light's plane, one byte per record, laid out by the shard
    uint32_t tile0, n_tiles, n_samples, scratch;
    uint32_t first;               // k_light_reduce: the first samples of these tiles (counts are set, not added to)
    TileGeom geom;
    uint32_t seed0;               // the seed of the chunk's first sample: frame0 + light_index * 64 + sample
    float shadow_eps;
    ViewDev view;
    trx_light light;
    uint32_t n_tris, n_inst;      // the extents of tris and inst_xform: what a caller's record may index (surface_record; last, as in AoRaysParams)
};
hipError_t launch_light_rays(const LightRaysParams &p, hipStream_t stream);
hipError_t launch_light_reduce(const LightRaysParams &p, hipStream_t stream);

// The light term (k_light_term): one lane per pixel of the shard's tiles, every buffer laid out by the shard; the lights
// by value, plane k of `lit` at k * plane_stride.
struct LightTermParams {
    const trx_hit *primary;
    const trx_hit_attr *attr;
    const uint8_t *lit;
    const trx_ao_term *term; // or null: the ambient is unoccluded
    float *value;
    uint32_t n_tiles, n_lights, n_samples, plane_stride;
    float ambient;
    TileGeom geom;
    ViewDev view;
    trx_light lights[TRX_MAX_LIGHTS];
};
hipError_t launch_light_term(const LightTermParams &p, hipStream_t stream);

// One-bounce indirect light (trx_bounce_light_rays_dev / trx_trace_indirect_dev; include/trx.h, "indirect light").  The
// bounce rays are k_ao_rays' (scratch layout, tmax = FLT_MAX), walked by the closest-hit rays launch and given attributes by
// k_hit_attr in rays mode; the kernels here work on those three buffers, indexed alike: in record layout (scratch == 0, one
// sample) by the pixel's record, in scratch layout by ((tile - tile0) * n_samples + sample) * 64 + pixel-in-tile.
//   k_bounce_light_rays  one lane per (tile, sample, pixel): the shadow ray from the bounce hit toward ONE light (by value)
//                        at rays[index]; the inert ray where the bounce found no surface or the hit faces away.
//   k_bounce_weight      one lane per (tile, sample, pixel): sum[index] (set to 0 for the first light) gets intensity * g
//                        added where the shadow ray was cast, flags[index] == 0 and g > 0.
//   k_bounce_gather      one lane per pixel of the chunk's tiles: acc[(tile - tile0) * 64 + pixel] (set to 0 for the first
//                        samples of the tiles) gets the chunk's sum[] added, samples ascending.
//   k_bounce_finish      one lane per pixel of the chunk's tiles: value[record] = base + (albedo * acc) / n_total, or base
//                        where the primary record is no surface (base: base[record], 0 with a null pointer).  The running sum
//                        sits in acc, not in value, so base may be value itself.
// k_bounce_light_rays and k_bounce_finish have a SPARSE instantiation (below, `stride`); k_bounce_weight and k_bounce_gather
// see the scratch alone and serve both forms.
// scratch per (tile, sample): the bounce rays, hits, instance ids, attributes and sums beside the AO pass's rays and flags,
// and the tile's 64 running sums (one set per tile: counted here per sample, which is at most what they take)
constexpr uint32_t kBounceUnitBytes = kAoUnitBytes + 64u * (32u + 8u + 4u + 24u + 4u + 4u);
struct BounceParams {
    const trx_ray *bounce_rays;
    const trx_hit *bounce_hits;
    const trx_hit_attr *bounce_attr;
    trx_ray *rays;                // the shadow rays (k_bounce_light_rays writes, k_bounce_weight reads)
    const uint8_t *flags;         // k_bounce_weight: the occlusion flags of the shadow rays
    float *sum;                   // k_bounce_weight, k_bounce_gather: s of every (tile, sample, pixel)
    float *acc;                   // k_bounce_gather, k_bounce_finish: A of every pixel of the chunk's tiles
    const trx_hit *primary;       // k_bounce_finish
    const float *base;            // k_bounce_finish, or null
    float *value;                 // k_bounce_finish
    uint32_t tile0, n_tiles, n_samples, scratch;
    uint32_t first;               // k_bounce_weight: the first light; k_bounce_gather: the first samples of these tiles
    uint32_t n_total;             // k_bounce_finish: the pass's n_samples
    TileGeom geom;
    uint32_t seed0;               // the seed of the chunk's first sample: frame0 + light_index * 64 + sample
    float shadow_eps, albedo;
    trx_light light;
    // sparse (trx_trace_indirect_sparse_dev; scratch layout, whole image; last: the fields above keep their offsets): the
    // tiles are those of the LOW grid `lo`, as AoRaysParams describes them.  k_bounce_light_rays takes its noise at the cell's
    // pixel (X * stride + px0, Y * stride + py0) of the full image `geom`; k_bounce_finish reads that pixel's primary record
    // and writes value[Y * lo.width + X] - +0 for a cell whose pixel leaves the image.  The dense launches leave stride 0.
    uint32_t stride, px0, py0;
    TileGeom lo;
    uint32_t n_tris;              // k_bounce_finish: the scene's triangle extent (surface_record: the surface as k_ao_rays decided it)
    // colour (trx_trace_indirect_rgb_dev / _rgb_sparse_dev; include/trx.h, rule 5c; last again: the fields above keep their
    // offsets): with `materials` set launch_bounce_gather and launch_bounce_finish run k_bounce_gather_rgb and
    // k_bounce_finish_rgb.  acc then holds three planes of n_tiles * 64 running sums (plane c at c * n_tiles * 64), value three
    // planes of `plane` floats (plane c at c * plane); base and albedo are not read.
    //   k_bounce_gather_rgb  one lane per pixel of the chunk's tiles: per sample of the chunk, where the bounce has a surface
    //                        (the ray's tmax, the hit), m = tri_material[hit.prim] and A_c = A_c + (albedo_c(m) * s + emission_c(m)).
    //   k_bounce_finish_rgb  one lane per pixel (SPARSE: cell) of the chunk's tiles: value[c * plane + record] = A_c / n_total,
    //                        +0 where the primary record is no surface.
    const trx_material *materials; // the scene's table, or null: the grey kernels
    const uint16_t *tri_material;  // n_tris indices into it, every one validated on upload
    uint32_t plane;                // floats per plane of value
    // emitters (trx_trace_indirect_rgb_emitters_dev / _sparse_dev; include/trx.h, rule 5e; last once more: the fields above
    // keep their offsets): with `emitters` set launch_bounce_emitter_rays runs k_bounce_emitter_rays after the chunk's lights
    // and launch_bounce_gather runs k_bounce_emitter_gather in k_bounce_gather_rgb's place.
    //   k_bounce_emitter_rays         one lane per (tile, sample, pixel): rules E2-E4 at the bounce hit (seed0 = frame0 + 8192 +
    //                                 the chunk's first sample) - the shadow ray at rays[index], wgeo (+0 where no ray was
    //                                 cast) at wgeo[index], the emitter at pick[index].
    //   k_bounce_emitter_gather  k_bounce_gather_rgb with rule 5e for 5c: s is sum[index] (+0 with has_lights == 0: no
    //                                 weight kernel wrote it), X_c = wgeo * emission_c(emitter) where wgeo > 0 and flags == 0.
    const float4 *emitters;        // the scene's emitter table (EmitterParams), or null: every other mode
    const float *cdf;
    float *wgeo;
    uint32_t *pick;
    uint32_t n_emitters, has_lights;
    float emitter_eps;
    // textures (trx_trace_indirect_rgb_textured_dev; include/trx.h, "THE TEXTURED ALBEDO"; last yet again: the fields above keep
    // their offsets): with tex.texcoords and tex.descs set launch_bounce_gather runs k_bounce_gather_tex<EMITTERS> in place of
    // k_bounce_gather_rgb / k_bounce_emitter_gather - the same rule with albedo_c(m) sampled at the bounce hit from
    // bounce_attr[index].  Null pointers: the kernels above.
    TextureTables tex;
};
hipError_t launch_bounce_emitter_rays(const BounceParams &p, hipStream_t stream);
hipError_t launch_bounce_light_rays(const BounceParams &p, hipStream_t stream);
hipError_t launch_bounce_weight(const BounceParams &p, hipStream_t stream);
hipError_t launch_bounce_gather(const BounceParams &p, hipStream_t stream);
hipError_t launch_bounce_finish(const BounceParams &p, hipStream_t stream);

// Emissive triangles as sampled lights (include/trx.h, "emitters").  The emitter table: four float4 per emitter, world space -
//   [0] V0.xyz, kinv    [1] E1.xyz, material index    [2] E2.xyz, prim    [3] NG.xyz, instance id (0xFFFFFFFF: single level)
// (the three indices as the bit patterns of the w lanes) - and the dense array c of n - 1 cumulative selection probabilities.
//   k_emitter_build   one lane per emitter: the (instance, prim) pair's 48-byte scene record, through the instance's
//                     object-to-world matrix (16 floats, column-major, as the refit takes them) where o2w is set; kinv is
//                     written as +0 - the host fills it in once it has the areas.
//   k_emitter_select  one lane per u0: emitter_select over caller-given values (trx_debug_emitter_select).
struct EmitterBuildParams {
    const float4 *tris;
    const float *o2w;              // or null: no instance transforms
    const uint2 *pairs;            // {instance id, prim} per emitter
    const uint16_t *tri_material;
    float4 *out;
    uint32_t n, n_tris, n_inst;    // the extents of pairs, tris and o2w (a pair outside them writes a zero record)
};
hipError_t launch_emitter_build(const EmitterBuildParams &p, hipStream_t stream);
struct EmitterSelectParams {
    const float *cdf;
    const float *u0;
    uint32_t *j;
    uint32_t n_emitters, n;
};
hipError_t launch_emitter_select(const EmitterSelectParams &p, hipStream_t stream);

// The emitter light pass at primary hits (trx_emitter_rays_dev / trx_trace_emitter_light_dev): the light visibility pass's
// shape with one "light", the table.  k_emitter_rays writes the shadow rays of rules E1-E4 - record layout or scratch layout
// exactly as AoRaysParams describes them, one lane per (tile, sample, pixel) - and, in scratch layout, wgeo (+0 where no ray
// was cast) and the selected emitter j beside them; the any-hit rays launch walks them; k_emitter_gather_rgb adds
// wgeo * emission_c(emitter j) of the samples that were cast and not occluded to three running sums per tile pixel (acc,
// plane c at c * n_tiles * 64; set for the first samples of the tiles), samples ascending, and with `last` writes
// value[c * plane + record] = base + A_c / n_total (base where the primary record is no surface; base read before value is
// written, by the same lane: they may be one buffer) instead of storing the sums.
// scratch per (tile, sample): rays, flags, wgeo and j, and the tile's 3 x 64 running sums (counted per sample, as in kBounceUnitBytes)
constexpr uint32_t kEmitterUnitBytes = kAoUnitBytes + 64u * (4u + 4u + 12u);
struct EmitterParams {
    const float4 *tris;
    const float4 *inst_xform;     // world-to-object rows per instance, or null (no instance transforms)
    const trx_hit *primary;
    const uint32_t *primary_inst; // read only with inst_xform
    trx_ray *rays;
    const uint8_t *flags;         // k_emitter_gather_rgb: the occlusion flags of the scratch rays
    const float4 *emitters;
    const float *cdf;
    const trx_material *materials;
    float *wgeo;                  // scratch layout only (null in record layout)
    uint32_t *pick;
    float *acc;
    const float *base;            // three planes like value, or null
    float *value;
    uint32_t tile0, n_tiles, n_samples, scratch;
    uint32_t first, last;         // k_emitter_gather_rgb: the first / the last samples of these tiles
    uint32_t n_total;             // the pass's n_samples
    TileGeom geom;
    uint32_t seed0;               // the seed of the chunk's first sample: frame0 + 2048 + sample
    float shadow_eps, emitter_eps;
    ViewDev view;
    uint32_t n_emitters, plane;   // floats per plane of value and base
    uint32_t n_tris, n_inst;      // the extents of tris and inst_xform: what a caller's record may index (surface_record)
};
hipError_t launch_emitter_rays(const EmitterParams &p, hipStream_t stream);
hipError_t launch_emitter_gather(const EmitterParams &p, hipStream_t stream);

// Resident waves the persistent kernel should be launched with on `device`.
int trace_grid_size(int device, int mode, bool tlas, uint32_t sem, bool count);

// Enqueues one traversal kernel.  sem: trx_semantics bits; pipe: the pipelined walk (BLAS-only scenes; ignored with a TLAS).
// (single-level kernels receive the TraceParams part of p)
hipError_t launch_trace(const TraceParamsTlas &p, int mode, bool tlas, uint32_t sem, bool count, bool pipe, int grid,
                        hipStream_t stream);

} // namespace trx
