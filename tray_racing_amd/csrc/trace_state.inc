// trace_state.inc - part of k_trace (kernels.hip), included as text inside the kernel: the wave's LDS carve-up and the per-lane
// ray slot, the drain's and the thin walk's state, counters.
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
    // one LDS region per wave of the workgroup; waves do not synchronise with each other (incoherent passes:
    // one barrier at the very start and a wait-free hand-over of rays between the two waves of a workgroup, see "The drain")
    extern __shared__ float4 lds_dyn[];
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave_in_block = threadIdx.x / kWave;
    // (a macro-like lambda, recomputed at each of its few uses - start-up, a tile filed, the epilogue - rather than a value
    // carried through the walk: the two-level AO kernel sits at the register budget)
    auto wave_id = [&]() -> uint32_t {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave));
    };
#define wave_global (wave_id())
    char *const lds_wave = reinterpret_cast<char *>(lds_dyn) + wave_in_block * kLdsBytesPerWave;
    lds_u32x2 *const lds_stack =                                                           // [kLdsStack][64], see lds_u32x2
        (lds_u32x2 *)((__attribute__((address_space(3))) char *)lds_dyn + wave_in_block * kLdsBytesPerWave);
    float4 *const lds_ray = reinterpret_cast<float4 *>(lds_wave + kLdsStack * kWave * 8);  // [64][2]: o,tmin | d
    uint2 *const lds_grp = reinterpret_cast<uint2 *>(lds_ray + 2 * kWave);                 // [64] triangle group of the lane
    uint2 *const lds_res = lds_grp + kWave;                                                // [64] {tt bits, triangle}
    uint32_t *const lds_pref = reinterpret_cast<uint32_t *>(lds_res + kWave);              // [64] first pair of the lane
    uint32_t *const lds_head = lds_pref + kWave;                                           // [64] run starts of a window
    uint2 *const lds_pend = reinterpret_cast<uint2 *>(lds_head + kWave);                   // [kLptPend] {tile, list} to append
    float *const lds_dec = reinterpret_cast<float *>(lds_pend + kLptPend);                 // [3][8][2] decoded child planes {min, max} of a wave-uniform node step
    float *const lds_dec_neg = reinterpret_cast<float *>(lds_head);                        // [3][8][2] the same as {max, min} (node_intersect_kept); shares lds_head
    float *const lds_cull = reinterpret_cast<float *>(lds_pref);                           // [8][2][4] per child {lower bounds of the near planes x y z -}{upper bounds of the far planes x y z -} of a packet test; shares lds_pref
    float4 *const lds_cull_rays = reinterpret_cast<float4 *>(lds_dec + 48);                // [3] per axis {lo, hi} of the wave's rays' 1/d, their common origin component, -: the packet test's constants
    // The wave's HBM area: stack entries past the LDS part, then the lanes' world-space rays ([6][64] floats, kernels.h).
    // Touched on rare paths only (a stack deeper than kLdsStack; entering and leaving an instance with a transform).  Its
    // base lives in two LANES of a vector register (the kernels hold more wave-uniform values than there are scalar
    // registers) and is read back on those paths - the 14 lane-spill instructions inside the primary kernel's walk loop
    // are these, none of them on a path a trip normally takes (tests/test_kernel_resources.py).  (The base formed on the
    // rare paths instead, from the kernel-argument segment: measured slower, profiles/r06_ab_lane_spills.log.)
    uint2 *const spill = P.spill + (size_t)wave_global * kWaveScratch;
#define wray (reinterpret_cast<float *>(spill + kSpillStack * kWave))
    const bool tie_first = P.tie_first != 0;
    if (P.wave_times && lane == 0) P.wave_times[kWaveTimeStride * wave_global] = wall_clock64();
    // (counting kernels, never timed: what refill_params() reads back IS this launch's parameter block - a second kernel
    // parameter or kernel-argument preloading would move it; a mismatch is reported as a failed launch)
    if (COUNT && lane == 0 && refill_params()->n_items != P.n_items) atomicAdd(&P.ctr->overflow, 1u);
    // (kTailDiag builds: what was every wave's LAST tile, and when did it start?  kStamps builds: phase cycles)
    unsigned long long diag_t0 = 0ull, diag_chunk = 0ull, diag_tiles = 0ull;
    uint32_t diag_dry_alive = 0u, diag_dry_age = 0u;
    unsigned long long diag_dry_t = 0ull;
    unsigned long long stamp_prev = kStamps ? __builtin_amdgcn_s_memtime() : 0ull;
    unsigned long long k_refill = 0, k_fetch = 0, k_test = 0, k_tri = 0, k_pop = 0, k_iters = 0;

    // per-lane ray slot
    bool has_ray = false;
    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = r.tmin = 0.0f;
    r.oct_inv4 = 0;
    float t = 0.0f;
    uint32_t prim = TRX_INVALID, out_index = 0, sp = 0, steps = 0;
    uint32_t trip = 0; // traversal-loop trips of this wave (uniform)
    uint32_t uni_cool = 0; // (uniform) trips for which the decode-once look is skipped
    // Packet culling of wave-uniform node steps (coherent primary rays, reciprocal arithmetic; two-level scenes: without
    // instance transforms - a ray keeps its world-space origin and direction inside an instance -;
    // kernels.hip node_intersect_kept, trace_walk_plain.inc): per axis the bounds of the wave's rays' 1/d and the rays'
    // common origin component, in LDS (lds_cull_rays; registers are what this kernel has least of), refreshed whenever the
    // wave takes new rays (trace_refill.inc).  cull_ok (wave-uniform): the rays share one origin and one direction
    // octant and every bound is finite.
    constexpr bool kCull = MODE == kModePrimary && !COUNT;
    bool cull_ok = false;
    uint32_t tlas_sp = TRX_INVALID, bvh_off = 0;
    // instance transforms (TLAS): the instance being walked / the one the current hit was found in, and the
    // world-space ray (origin, direction as given) to come back to when the BLAS is left
    uint32_t cur_inst = TRX_INVALID, hit_inst = TRX_INVALID;
    uint2 cur = make_uint2(0u, 0u);
    // pipelined walk: node in flight / fetched for this lane, and the triangle group its last node test left
    bool fetched = false;
    uint4 pn0 = make_uint4(0u, 0u, 0u, 0u), pn1 = pn0, pn2 = pn0, pn3 = pn0, pn4 = pn0;
    uint2 ptri = make_uint2(0u, 0u);
    uint32_t overflow = 0; // sticky, set on the rare paths only (stack past its HBM part, step cap)
    // kModeFused (the reference's one-dispatch frame, rt_gpu_software.hlsl:47-144): a lane whose primary ray has ended in
    // a hit keeps t / prim / out_index and waits (`pend`) until the wave next refills; it is then turned into that pixel's
    // AO ray in place (`is_ao`), together with every other waiting lane and with the lanes that take new pixels - one
    // pass through the ray set-up code for all of them, not one per finished ray
    constexpr bool kFused = MODE == kModeFused;
    bool pend = false, is_ao = false;
    // The drain (incoherent single-level passes - AO, explicit rays - run two waves to a workgroup).  Every wave of such a pass finds the queues dry
    // holding about 45 rays and then spends a full ray lifetime finishing them at falling occupancy (13 % of a
    // bistro-class AO pass, 64 % of a hairball-class one: profiles/r03_ao_order.log).  Fewer waves draining is the remedy:
    // once the two waves of a workgroup are both dry and their rays fit one wave, the second wave parks its rays' state
    // in its own (now idle) LDS region, offers them with one LDS compare-and-swap and leaves; the first wave picks them
    // up into its idle lanes - stack entries included, they are in the same workgroup's LDS - and goes on.  A ray is
    // the same ray whichever wave steps it, so the hits are those of the unmerged pass.  No wave ever waits for the other:
    // control word 0 goes 0 -> n (rays offered) or 0 -> kMergeClosed (the first wave left first), whichever swap lands.
    // (Single-level walks, and explicit rays over two-level scenes - ten words more per ray, 32 rays at most.  The two-level AO kernel
    // that contains the code is 2.5-3 % slower on the 4K pass than the one that does not, profiles/r03_drain_merge.log,
    // r05_ab_5_tlas.log: compiled out there.)
    // Thin waves (incoherent single-level passes, queues dry, at most P.thin_max rays left): eight lanes to a ray, see thin_walk.
    constexpr bool kThin = !TLAS && MODE != kModePrimary && !COUNT;
    bool go_thin = false; // wave-uniform
    // (two-level walks: explicit rays only - measured on the 4K two-level scene, profiles/r05_ab_5_tlas.log: rays -4 %, AO pass +2.5 %)
    constexpr bool kMerge = (!TLAS || MODE == kModeRays) && MODE != kModePrimary && MODE != kModeFused && MODE != kModeService && !COUNT;
    constexpr uint32_t kMergeWords = TLAS ? 31u : 21u, kMergeMax = TLAS ? 32u : 48u, kMergeClosed = 0xffffffffu;
    const bool merging = kMerge && P.merge != 0u && blockDim.x == 2u * kWave;
    bool merge_open = merging; // wave-uniform: this wave has not offered / taken / refused rays yet
    uint32_t need_take = 0u;   // wave-uniform: rays the first wave found offered as it was about to leave
    char *const lds_wave0 = reinterpret_cast<char *>(lds_dyn), *const lds_wave1 = lds_wave0 + kLdsBytesPerWave;
    // control words (in wave 0's decode table, which only coherent primary passes use): [0] offer, [1] free lanes of wave 0
    uint32_t *const merge_ctl = reinterpret_cast<uint32_t *>(lds_wave0 + (reinterpret_cast<char *>(lds_dec) - lds_wave));
    // parking area: wave 1's region from its ray copies up to and including its decode table (4 032 B = 48 x 21 words)
    uint32_t *const merge_box = reinterpret_cast<uint32_t *>(lds_wave1 + kLdsStack * kWave * 8);
    const uint2 *const merge_stack1 = reinterpret_cast<const uint2 *>(lds_wave1);
    if (merging) {
        if (threadIdx.x == 0u) {
            merge_ctl[0] = 0u;
            merge_ctl[1] = 0u;
        }
        __syncthreads(); // (the only barrier of the kernel: both waves are at their very start)
    }
    // kModeService (kernels.h, kSvcRays): the mailboxes between the workgroup's porter wave and its walker wave live in the
    // porter's LDS region - per ray slot g: words [16 g .. 16 g + 8] = the request {ox oy oz dx dy dz tmin tmax} and [16 g + 12]
    // its sequence number (porter -> walker); words [128 + 4 g ..] = the answer {t, prim, overflow, seq} (walker -> porter);
    // word [192] != 0: leave.  svc_seq (per lane, the same in a group's eight lanes): the request the group last accepted.
    // (an LDS pointer, like the stacks': through a generic pointer every look into a mailbox was a `flat_load ... sc0 sc1`
    // followed by `s_waitcnt vmcnt(0)` - the walker's step (0) then waited, every trip, for every node, triangle and touch
    // request in flight: 1.5 us a trip whatever the caches held, profiles/r06_ray_service.log)
    typedef volatile __attribute__((address_space(3))) uint32_t svc_word;
    svc_word *const svc_box = (svc_word *)((__attribute__((address_space(3))) char *)lds_dyn + kLdsBytesPerWave);
    uint32_t svc_seq = 0u;
    unsigned long long svc_t0 = 0ull; // (when the group's ray was accepted)
    // COUNT only
    uint32_t c_node = 0, c_tri = 0, c_rays = 0, c_hits = 0, c_maxsp = 0, c_over = 0;
    uint32_t c_wnode = 0, c_wtri = 0; // wave-level executions (leader lane only): SIMD-efficiency denominators
    uint32_t s_wnode = 0, s_wtri = 0; // their values when the current tile started
    // per-ray counts (SlotCounters::ray_cost): a counting kernel has no thin waves, no ray merging and no drain, so a ray keeps
    // its lane from the refill that publishes it to finish_lane, and cooperative triangle rounds credit their tests to the
    // owning lane - a ray's own node visits and triangle tests are what the lane's counters gained in between
    trx_ray_cost *const ray_cost = COUNT ? P.ctr->ray_cost : nullptr;
    uint32_t r_node = 0, r_tri = 0; // c_node / c_tri when the lane's ray was published

