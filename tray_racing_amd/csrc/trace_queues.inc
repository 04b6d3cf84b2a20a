// trace_queues.inc - part of k_trace (kernels.hip), included as text inside the kernel: the work queues and the tile order a frame reads
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
    // ---- work queues ---------------------------------------------------------------------
    // Work is cut into chunks of 64 items (one 8x8 tile, or 64 explicit rays).  Chunk p belongs
    // to queue p % 8 (ticket k of queue q is chunk 8k + q); a wave pulls from the queue of the XCD
    // it runs on (one atomic head per XCD: a single head saturates near 90 dequeues/us) and
    // steals from the other queues when its own runs dry.  The next ticket is taken when it is needed
    // (heavy tiles, passes without an order) or a tile ahead (light tiles of an ordered frame), see below.
    //
    // Tile order: a wave that finishes a tile of a LEARNING frame (the first frame of a view; every frame of
    // a moving camera) files it in one of 16 cost buckets (sqrt(2)-wide classes of the tile's traversal-loop
    // trips) of the other list set; a frame reads the set on file heaviest bucket first, so chunk p is the p-th
    // heaviest tile (longest-processing-time-first) and every queue starts with heavy tiles - and while the
    // view stays the same it reads that set unchanged and files nothing (`frozen`, below).
    const uint32_t n_chunks = (P.n_items + 63u) >> 6;
    uint32_t my_q = P.single_queue ? 0u : (read_xcc_id() & 7u);
    uint32_t q_probes = 0;
    uint32_t pending = 0; // prefetched ticket of queue my_q (lane 0)
    bool have_pending = true; // uniform: a ticket of queue my_q is in flight / held in `pending`
    if (lane == 0) pending = atomicAdd(&P.ctr->heads[my_q].taken, 1u);
    uint32_t chunk_next = 0, chunk_left = 0; // items of the current chunk not yet handed to a lane
    uint32_t n_pend = 0;                     // tile-list entries parked in lds_pend (uniform)
    uint32_t tile_slot = TRX_INVALID;        // tile being timed (cost feedback)
    unsigned long long tile_t0 = 0;
    uint32_t tile_trip0 = 0;
    uint32_t cur_tile = 0, my_tile = 0;      // tile of the current chunk (uniform) / of this lane's item
    uint32_t cur_vf = 0, my_vf = 0;          // AO batches: frame (noise seed) of the current chunk (uniform) / of this lane's item
    // Lists are kept per (cost bucket, shard): kLptShards appenders per bucket (a wave always appends to its own shard), because one atomic
    // word saturates near 90 appends/us.  Entry e = (15 - bucket) * kLptShards + shard is the e-th
    // list of the heaviest-first concatenation; lane l holds the (exclusive) ends of entries l, l+64.
    uint32_t end_a = 0, end_b = 0;
    bool ordered = false;
    // The feedback machinery tunes itself (exit protocol below): a slot whose frames measured faster WITHOUT it runs without
    // it - natural order, no tile timing, no list appends - until the next re-evaluation.  Every wave reads the same word.
    // (the host files an order for primary and one-seed AO passes only: explicit-ray batches and one-launch frames carry none of this)
    constexpr bool kOrder = MODE != kModeRays && MODE != kModeService;
    const uint32_t fb_mode = (kOrder && P.fb != nullptr && !P.new_view) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.fb->mode) : 0u;
    const bool fb_off = fb_mode != 0u;
    // (mode 2: a frame whose tiles are ragged - a few rays of a tile run ten times longer than the rest - keeps its lanes
    // busier by replacing finished rays mid-tile; one frame per launch only, the frame of a batch is taken from whole tiles)
    constexpr uint32_t kFbRefill = 16u;
    const uint32_t refill_idle = (fb_mode == 2u && P.n_frames == 1u) ? kFbRefill : P.refill_idle;
    if (kOrder && P.fb && wave_global == 0u && lane == 0u) P.fb->t0 = wall_clock64(); // (about when the frame's first waves start)
    // The order lives in one of two list sets; the word *lpt_sel (flipped by the exit wave of a frame that filed a new
    // order) says which one is read.  The other set is empty and takes what this frame files - unless the frame finds a
    // COMPLETE order and its views are the previous frame's (same_view): then the order is frozen - replayed as it is, no
    // tile is timed, nothing is filed, the set stays.  Measured (profiles/r04_order_dynamics.log): an order that keeps
    // being rewritten from each frame's completion order wanders - the shards deal a class out to eight lists and
    // concatenate them again, a permutation with short cycles: frame times settle over 10-30 frames or alternate between
    // two values 5 % apart - while the order filed by the very FIRST frame of a view, frozen, runs 1 % faster than the
    // settled one from its second frame on (bistro-class frame 0.420 against 0.425 ms; the filing machinery is off too).
    const bool have_lists = kOrder && P.lpt_sets != nullptr;
    const uint32_t lpt_rd = (have_lists && __builtin_amdgcn_readfirstlane((int)*P.lpt_sel) != 0) ? P.lpt_set_words : 0u;
    uint32_t *const rd_set = P.lpt_sets + lpt_rd, *const wr_set = P.lpt_sets + (P.lpt_set_words - lpt_rd);
    const uint32_t *const rd_lists = rd_set + 16u * kLptShards;
    if (have_lists && !fb_off && !P.no_order) {
        end_a = rd_set[(15u - (lane >> 3)) * kLptShards + (lane & 7u)];
        end_b = rd_set[(15u - ((lane + 64u) >> 3)) * kLptShards + (lane & 7u)];
        // a list that overflowed its capacity dropped entries: fall back to the natural order
        const bool intact = __ballot(end_a > P.lpt_cap || end_b > P.lpt_cap) == 0ull;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t ya = __shfl_up(end_a, off), yb = __shfl_up(end_b, off);
            if ((int)lane >= off) {
                end_a += ya;
                end_b += yb;
            }
        }
        end_b += (uint32_t)__builtin_amdgcn_readlane((int)end_a, 63);
        ordered = intact && (uint32_t)__builtin_amdgcn_readlane((int)end_b, 63) == n_chunks; // complete lists
    }
    const bool frozen = ordered && P.same_view != 0u;
    // (through readfirstlane: a wave-uniform flag that lives to the epilogue belongs in a scalar register)
    const bool lpt_write = __builtin_amdgcn_readfirstlane((have_lists && !fb_off && !frozen) ? 1 : 0) != 0;

    // Chunks below this index of the heaviest-first order take their successor's ticket LATE (when the wave is idle), the
    // rest a tile ahead (hides the atomic's 1-2 us round trip, which only matters next to a tile of a few us).  Round 2
    // cut the order in half by position (never / always / heaviest 3 % / 12 % / 50 %, profiles/r02_late_binding.log);
    // round 3 looked at what the last waves out of a frame had been doing: starting a 20-30 us tile
    // they had reserved a tile earlier, while hundreds of idle waves found the queues dry and left - the position cut
    // sits in the middle of the 20-40 us tiles of the bistro-class frame.  The cut is a class now: tiles of 16 trips or more (class 7 and up, about 35 us mid-frame) bind late (profiles/r03_tile_classes.log:
    // classes 6..9 within 1 % of each other, all ahead of the position cut).
    constexpr uint32_t kLateClass = 7u;
    constexpr uint32_t late_entry = (15u - kLateClass) * kLptShards + (kLptShards - 1u); // last list of that class in the concatenation
    uint32_t late_cut = 0u;
    if (ordered)
        late_cut = late_entry < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)end_a, (int)late_entry)
                                    : (uint32_t)__builtin_amdgcn_readlane((int)end_b, (int)(late_entry - 64u));
    // ... and so do the last tiles of the order, half as many as there are waves: a ticket reserved a tile ahead there is a
    // tile that an idle wave could have started (profiles/r03_tile_classes.log section 9: 0 / 1024 / 2048 / 4096 / 8192
    // tiles with 4096 waves; kitchen-class -2 %, bistro-class -1 %, the others unchanged up to 2048, slower beyond)
    const uint32_t tail_tiles = (gridDim.x * (blockDim.x / kWave)) >> 1;
    const uint32_t tail_cut = n_chunks > tail_tiles ? n_chunks - tail_tiles : 0u;
    bool exhausted = false; // wave-uniform
