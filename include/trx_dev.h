/* trx_dev.h - development surface of libtrx.so: diagnostics and tuning switches used by tools/, bench.py's legs and
 * the tests.  NOT part of the drop-in boundary: nothing here replaces an interface of tray_racing, INTEGRATION.md binds
 * none of it, and a host that only includes trx.h never sees it.  Results of every trace entry point are identical
 * whatever is set here (tests/test_gpu_parity.py::test_scheduling_variants_and_streams_do_not_change_results). */
#ifndef TRX_DEV_H
#define TRX_DEV_H

#include "trx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics: start / end wall-clock stamps (100 MHz ticks) of every persistent wave of one
 * primary frame: out_times[2*i], out_times[2*i+1].  Shows residency and the frame's tail. */
int trx_debug_wave_timeline(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                            uint32_t semantics, uint64_t *out_times, uint32_t max_waves,
                            uint32_t *out_waves);

/* Diagnostics: 8 words per wave: start, end (as above), then — only in libraries built with -DTRX_STAMPS,
 * zero otherwise — shader cycles spent in {refill, node fetch, node test, triangle phase, pop / bookkeeping}
 * and the number of loop trips. */
int trx_debug_wave_phases(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                          uint32_t semantics, uint64_t *out_records, uint32_t max_waves,
                          uint32_t *out_waves);
/* The same 8-word records for the AO pass of the frame (frame 0, eps 0.01; its primary pass runs first, unrecorded). */
int trx_debug_wave_timeline_ao(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                               uint32_t semantics, uint64_t *out_records, uint32_t max_waves,
                               uint32_t *out_waves);

/* Diagnostics (counting kernel): the compulsory footprint of one primary frame — how many distinct nodes were
 * fetched and distinct triangles tested (80 * nodes + 48 * tris + 8 * rays bytes). */
int trx_debug_footprint(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                        uint32_t semantics, uint64_t *out_nodes_touched, uint64_t *out_tris_touched);

/* Diagnostics (counting kernel): over the triangle phases of one primary frame, out_hist[0..15] = histogram of the
 * largest per-lane triangle count of the wave (15 = 15 or more), out_hist[16..31] = histogram of the wave's
 * (ray, triangle) pair total in units of 8, rounded up. */
int trx_debug_tri_histogram(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                            uint32_t semantics, uint32_t out_hist[32]);

/* Diagnostics: per 8x8 tile (row-major tile id) the wall-clock cost of the tile in a normal frame
 * (100 MHz ticks) and its wave-level iteration counts from a counting frame:
 * (node steps << 16) | triangle rounds.  n_tiles = ceil(w/8) * ceil(h/8). */
int trx_debug_tile_profile(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                           uint32_t semantics, uint32_t *out_cost, uint32_t *out_iters, uint32_t n_tiles);

/* Launches issued and rays served by trx_traverse1 on this scene so far: the ray services' kernel starts (a handful per
 * stretch of calls).  Either pointer may be NULL. */
int trx_debug_traverse1_stats(trx_scene *scene, uint64_t *out_launches, uint64_t *out_rays);

/* The ray services of the scene (a resident kernel answers trx_traverse1, include/trx.h) so far: calls
 * answered, kernel starts, nanoseconds callers spent between posting a ray and reading its answer, the GPU-side share of
 * that in 100 MHz ticks (admission to answer) and the trips of the walks.  Any pointer may be NULL. */
int trx_debug_service_stats(trx_scene *scene, uint64_t *out_rays, uint64_t *out_starts, uint64_t *out_call_ns,
                            uint64_t *out_walk_ticks, uint64_t *out_walk_trips);

/* The scene's derived launch words as the kernels get them: exp_exact (0, 1 or 2: which exact shortcuts the node test may
 * take, trx_scene_create / trx_scene_refit derive it from the node bytes), the scene diagonal that scales camera-cut
 * detection, and the number of height levels of the refit's cached schedule (0 before the first refit).  Any pointer may
 * be NULL. */
int trx_debug_scene_info(trx_scene *scene, uint32_t *out_exp_exact, float *out_scene_diag, uint32_t *out_refit_levels);

/* Which walk the shipped library launches for a trace mode on this scene: 0 = the plain walk, 1 = the pipelined walk
 * (the next node's fetch issued under the triangle phase; single-level scenes past 32 MiB of nodes and triangle records,
 * every mode but the primary pass and the ray service).  mode: 0 primary, 1 AO (its batch and counting passes too), 2 explicit
 * rays (closest hit, any hit, trx_traverse_batch, the AO visibility passes), 3 the one-launch frame, 4 the ray service behind
 * trx_traverse1.  This is the decision the launch path itself takes; the forcing bits of development builds (TRX_DEV_TUNE)
 * are not reported.  A negative return is an error code. */
int trx_debug_walk_kind(trx_scene *scene, uint32_t mode);

/* Measuring aid: the reference's CPU pixel loop over the literal Traversable::traverse (src/rt_cpu/rt_cpu.rs:35-57) -
 * `threads` host threads, thread k calls trx_traverse1 for rays k, k + threads, ... - with the loop's wall-clock seconds and
 * the launches its calls shared. */
int trx_debug_traverse1_threads(trx_scene *scene, const trx_ray *rays, uint64_t n_rays, uint32_t threads, uint32_t semantics,
                                trx_rayhit *out, double *out_seconds, uint64_t *out_launches);

/* Measuring aid: the no-locality rate of the node-fetch loop on THIS scene's buffers (bench.py's `fetch_vs_random`).  The tracer's
 * persistent grid at the tracer's occupancy, every lane fetching one uniformly random 80-byte node per step and, on average,
 * tris_per_node_x256 / 256 random 48-byte triangle records beside it, the next index a hash of what arrived (one step in
 * flight per wave, like a traversing wave) - and nothing else.  Returns nodes and triangle records fetched per second. */
int trx_debug_fetch_rate(trx_scene *scene, uint32_t steps, uint32_t tris_per_node_x256, double *out_nodes_per_s,
                         double *out_tris_per_s);

/* Measuring aid: the streaming ceiling of this GPU's memory - a float4 copy kernel over `bytes` (read + written bytes per
 * second, best of `reps` passes after two warm-up passes): bench.py's `roofline_hbm.peak_measured`. */
int trx_debug_copy_rate(int device, uint64_t bytes, uint32_t reps, double *out_bytes_per_s);

/* AO visibility (trx_trace_ao_visibility_dev, include/trx.h): the cap, in bytes, on the ray scratch of a launch slot for
 * passes that start after the call (process-wide; 0 restores the default of 288 MiB).  Returns the previous cap.  Counts
 * are identical under every cap: a small one makes small images run the chunk loops (the test suite does that). */
uint64_t trx_debug_ao_scratch_cap(uint64_t bytes);
/* Measuring aid: one whole-image trx_trace_ao_visibility_dev pass on the null stream with hipEvents around the three
 * phases of every chunk; out_ms = {ray generation, any-hit walk, reduce} summed over the chunks.  Synchronous. */
int trx_debug_ao_visibility_phases(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                   uint32_t semantics, uint32_t frame0, uint32_t n_samples, float ao_eps, float ao_radius,
                                   const trx_hit *d_primary, const uint32_t *d_primary_inst, uint8_t *d_unoccluded,
                                   float out_ms[3]);
/* The same for one whole-image trx_trace_light_visibility_dev pass; out_ms summed over the lights and their chunks. */
int trx_debug_light_visibility_phases(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height,
                                      uint32_t semantics, uint32_t ray_mask, const trx_light *lights, uint32_t n_lights,
                                      uint32_t frame0, uint32_t n_samples, float shadow_eps, const trx_hit *d_primary,
                                      const uint32_t *d_primary_inst, uint8_t *d_lit, float out_ms[3]);
/* One whole-image trx_trace_indirect_dev pass on the null stream (synchronous), hipEvents around its launches; out_ms summed
 * over the chunks and lights: [0] the bounce rays, [1] the closest-hit walk over them, [2] their attributes, [3] the shadow
 * rays, [4] the any-hit walk over them, [5] weight, gather and finish. */
int trx_debug_indirect_phases(trx_scene *scene, const trx_view *view, uint32_t width, uint32_t height, uint32_t semantics,
                              uint32_t ray_mask, const trx_light *lights, uint32_t n_lights, uint32_t frame0,
                              uint32_t n_samples, float bounce_eps, float shadow_eps, float bounce_albedo,
                              const trx_hit *d_primary, const uint32_t *d_primary_inst, const float *d_base,
                              float *d_value, float out_ms[6]);

/* Diagnostics: the scheduling state of the launch slot whose last launch ran on `stream` - what decides in which order,
 * and by which schedule, the next image pass of `kind` (0 primary, 1 AO) on that stream deals out its tiles.  Hits never
 * depend on it; the tests read it to know that the state they claim to exercise (an order learnt, replayed frozen,
 * refiled, dropped; a tuner phase) was really reached. */
typedef struct trx_schedule_state {
    uint32_t have_slot;  /* a launch slot of the scene was last used by `stream` (everything below is 0 otherwise) */
    uint32_t slot;       /* ... its index */
    uint32_t have_lists; /* the slot holds tile lists of this kind (0: capacity .. other_sum, key are 0) */
    uint32_t capacity;   /* tiles the lists are sized for */
    uint32_t lpt_cap;    /* entries one of the 128 lists holds */
    uint32_t lpt_sel;    /* which of the two list sets is on file (read by the next frame) */
    uint32_t count_sum;  /* the set on file: sum of its 128 counts */
    uint32_t n_over;     /* ... and how many of them exceed lpt_cap (a list that dropped entries) */
    uint32_t other_sum;  /* sum of the 128 counts of the other set (0 between frames: it takes the next new order) */
    uint32_t mode, frames, phase; /* the schedule tuner: mode the next frame runs in, frames of the phase so far, phase 0..3 */
    uint64_t key;        /* the image geometry the order on file was learnt for (opaque; 0 = none) */
} trx_schedule_state;
/* Waits for `stream`, then fills *out and, with out_order non-null, writes the tile ids of the set on file in the order a
 * frame reads them - lists (15 - b) * 8 + shard for b = 0..15, shard = 0..7, concatenated, each cut at lpt_cap - up to
 * max_tiles of them (the rest of out_order is left alone).  Changes no state: neither the slot's nor the device's. */
int trx_debug_schedule_state(trx_scene *scene, void *stream, uint32_t kind, trx_schedule_state *out, uint32_t *out_order,
                             uint32_t max_tiles);

/* Emitters (include/trx.h, "emitters"): the device's selection function over n caller-given u0 values (device memory), one
 * uint32 j per value at d_j; on the null stream, synchronous.  It holds the search to the counting rule at every c_i itself,
 * not only at the values the hash happens to reach.  Refused like every emitter entry point (no table, a stale one). */
int trx_debug_emitter_select(trx_scene *scene, const float *d_u0, uint64_t n, uint32_t *d_j);

/* Kernel variant selection (tuning aid; 0 = default).  Returns the previous
 * value.  Variants compute identical results. */
uint32_t trx_set_kernel_variant(uint32_t variant);

#ifdef __cplusplus
}
#endif

#endif /* TRX_DEV_H */
