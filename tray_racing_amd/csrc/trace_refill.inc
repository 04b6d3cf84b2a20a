// trace_refill.inc - part of k_trace (kernels.hip), included as text inside the kernel: the top of the outer loop - tiles are filed, idle lanes get new rays
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
        // ---- refill idle lanes from the queues --------------------------------------------
        const unsigned long long idle = __ballot(!has_ray);
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (tile_slot != TRX_INVALID && n_idle == (uint32_t)kWave) {
            // the whole tile is done: record what it cost (feeds the next frame's tile order)
            if (lane == 0) {
                const uint32_t c = (uint32_t)(wall_clock64() - tile_t0);
                if (P.cost) P.cost[tile_slot] = c;
                if (lpt_write) {
                    // The tile's class for the next frame's order = its WORK, in half-octaves of traversal-loop trips (1, 2,
                    // 3, 4, 6, 8 ... 256+), not its duration.  How long a tile takes depends on when it ran - at the start
                    // of the frame with issue priority, mid-frame against four waves a SIMD, in the tail against none - so
                    // a frame ordered by last frame's durations reshuffles itself every frame (static camera: 43 % of the
                    // tiles moved by two duration classes or more from one frame to the next); trips
                    // are a property of the tile and the view, the same every frame.  A least-squares fit of mid-frame tile
                    // time on trips, per-lane triangle rounds and cooperative rounds explains no more than trips alone
                    // (residual 28.8 against 29.4 us rms), and classes of weighted work measured slower, so: trips.
                    // profiles/r03_tile_classes.log: hairball-class frame -6 %, dense -1.8 %, bistro-class -1.5 %.
                    const uint32_t wk = max(trip - tile_trip0, 1u);
                    const uint32_t msb = 31u - (uint32_t)__clz((int)wk);
                    const uint32_t kk = 2u * msb + (msb ? (wk >> (msb - 1u)) & 1u : 0u);
                    const uint32_t b = kk == 0u ? 0u : min(kk - 1u, 15u);
                    const uint32_t list = b * kLptShards + (wave_global & (kLptShards - 1u)); // (one shard per wave: see flush_pending)
                    // park the entry in LDS: the appends (returning atomics) are issued together,
                    // one lane each, when the buffer fills or the wave exits, off every tile's path
                    lds_pend[n_pend] = make_uint2(tile_slot, list);
                }
            }
            if (lpt_write) {
                n_pend++;
                if (n_pend == (uint32_t)kLptPend) {
                    flush_pending_plain(P, wr_set, lds_pend, n_pend, lane);
                    n_pend = 0;
                }
            }
            if (COUNT && P.tile_iters) {
                // wave-level node steps and triangle rounds of this tile (each is counted by one lane)
                uint32_t dn = c_wnode - s_wnode, dt = c_wtri - s_wtri;
                for (int off = 32; off > 0; off >>= 1) {
                    dn += __shfl_xor(dn, off);
                    dt += __shfl_xor(dt, off);
                }
                if (lane == 0) P.tile_iters[tile_slot] = (min(dn, 65535u) << 16) | min(dt, 65535u);
            }
            tile_slot = TRX_INVALID;
        }
        // (fused frames: lanes waiting to become AO rays are idle but take no new pixel)
        const unsigned long long freem = kFused ? (idle & ~__ballot(pend)) : idle;
        const uint32_t n_free = kFused ? (uint32_t)__popcll(freem) : n_idle;
        const bool take = !exhausted && n_idle >= refill_idle;
        if (take || (kFused && freem != idle)) {
            const uint32_t rank = lane_rank(freem);
            uint32_t given = 0, item = TRX_INVALID;
            while (take && given < n_free) {
                if (chunk_left == 0u) {
                    // take the prefetched ticket; walk to the next queue when this one is dry
                    if (!have_pending && lane == 0) pending = atomicAdd(&P.ctr->heads[my_q].taken, 1u);
                    uint32_t ticket = __builtin_amdgcn_readfirstlane(pending);
                    uint32_t q_count = P.single_queue ? n_chunks : ((n_chunks + 7u - my_q) >> 3);
                    while (ticket >= q_count) {
                        if (++q_probes >= (P.single_queue ? 1u : 8u)) break;
                        my_q = (my_q + 1u) & 7u;
                        if (lane == 0) pending = atomicAdd(&P.ctr->heads[my_q].taken, 1u);
                        ticket = __builtin_amdgcn_readfirstlane(pending);
                        q_count = (n_chunks + 7u - my_q) >> 3;
                    }
                    if (ticket >= q_count) {
                        exhausted = true;
                        if constexpr (kTailDiag) {
                            diag_dry_t = wall_clock64();                                 // when the wave found every queue dry ...
                            diag_dry_alive = (uint32_t)__popcll(__ballot(has_ray));      // ... how many rays it still held ...
                            uint32_t age = has_ray ? trip - steps : 0u;                  // ... and the age of the oldest, in trips
                            for (int off = 32; off > 0; off >>= 1) age = max(age, (uint32_t)__shfl_xor((int)age, off));
                            diag_dry_age = age;
                        }
                        break;
                    }
                    // a ticket taken a tile ahead hides the atomic's round trip (1-2 us) but binds the wave's NEXT tile
                    // while it still works on this one: a wave stuck on a 0.3 ms tile then sits on a second one that an idle
                    // wave could have started.  Late binding wins wherever tiles are long or of unknown cost - the heavier
                    // half of the heaviest-first order, and every pass that has no learnt order (first frame, AO, explicit
                    // rays); only the light half of an ordered frame keeps the prefetch
                    have_pending = ordered && ticket * (P.single_queue ? 1u : 8u) >= late_cut && ticket * (P.single_queue ? 1u : 8u) < tail_cut;
                    if (have_pending && lane == 0) pending = atomicAdd(&P.ctr->heads[my_q].taken, 1u);
                    const uint32_t chunk = P.single_queue ? ticket : ticket * 8u + my_q;
                    chunk_next = chunk << 6;
                    chunk_left = min(64u, P.n_items - chunk_next);
                    cur_tile = chunk;
                    if (MODE == kModeAo && P.n_frames > 1u) {
                        // AO batch (one view, one primary hit buffer, n_frames noise seeds - configs[3]'s "4 spp"): the
                        // seeds of a tile are consecutive tickets of ONE queue, so the same XCD walks the same origins
                        // through the same upper nodes n_frames times over; a tile id past the image is the padding of
                        // the last group of eight tiles (every queue has the same number of tickets)
                        const uint32_t tq = div_uniform(ticket, P.n_frames, P.rcp_n_frames);
                        cur_vf = ticket - tq * P.n_frames;
                        cur_tile = P.single_queue ? tq : tq * 8u + my_q;
                        if (cur_tile >= P.tiles_per_frame) {
                            chunk_left = 0u;
                            continue;
                        }
                    }
                    if (ordered) {
                        // chunk -> bucket (heaviest first) -> tile
                        uint32_t j = (uint32_t)__popcll(__ballot(chunk >= end_a));
                        if (j == 64u) j += (uint32_t)__popcll(__ballot(chunk >= end_b));
                        const uint32_t start = j == 0u ? 0u
                                               : j <= 64u ? (uint32_t)__builtin_amdgcn_readlane((int)end_a, (int)(j - 1u))
                                                          : (uint32_t)__builtin_amdgcn_readlane((int)end_b, (int)(j - 65u));
                        const uint32_t list = (15u - (j >> 3)) * kLptShards + (j & 7u);
                        cur_tile = rd_lists[(size_t)list * P.lpt_cap + (chunk - start)];
                        cur_tile = __builtin_amdgcn_readfirstlane(cur_tile);
                        if (cur_tile >= n_chunks) cur_tile = chunk; // (only a corrupted list can name such a tile: never turn it into an out-of-range pixel)
                        // the tiles that set the frame's critical path get issue priority over the
                        // waves they share a SIMD with
                        if (chunk < P.prio_cut[0]) __builtin_amdgcn_s_setprio(3);
                        else if (chunk < P.prio_cut[1]) __builtin_amdgcn_s_setprio(2);
                        else if (chunk < P.prio_cut[2]) __builtin_amdgcn_s_setprio(1);
                        else __builtin_amdgcn_s_setprio(0);
                    }
                    if ((P.cost || lpt_write) && n_idle == (uint32_t)kWave && given == 0u) {
                        tile_slot = cur_tile; // cost is filed under the tile, not the chunk
                        tile_t0 = wall_clock64();
                        tile_trip0 = trip;
                        if constexpr (kTailDiag) {
                            diag_t0 = tile_t0;
                            diag_chunk = chunk;
                            diag_tiles++;
                        }
                        s_wnode = c_wnode;
                        s_wtri = c_wtri;
                    }
                }
                const uint32_t n_take = min(n_free - given, chunk_left);
                if (rank >= given && rank < given + n_take) {
                    item = chunk_next + (rank - given);
                    my_tile = cur_tile;
                    if (MODE == kModeAo) my_vf = cur_vf;
                }
                chunk_next += n_take;
                chunk_left -= n_take;
                given += n_take;
            }
            const bool conv = kFused && pend; // this lane's primary ray hit something: it becomes the pixel's AO ray
            if (kFused && pend) item = TRX_INVALID; // (a waiting lane has no rank among the free ones)
            if (!has_ray && (item != TRX_INVALID || conv)) {
                bool ok = false;
                float dx = 0.0f, dy = 0.0f, dz = 0.0f;
                if (MODE == kModeRays) {
                    const float4 *rp = reinterpret_cast<const float4 *>(P.rays + item);
                    const float4 a = rp[0], b = rp[1];
                    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.tmin = a.w;
                    dx = b.x; dy = b.y; dz = b.z;
                    t = fminf(b.w, TRX_F32_MAX);
                    out_index = item;
                    ok = true;
                } else {
                    // The launch parameters only a refill needs - the view, the image geometry, the primary hits - are read from
                    // the kernel-argument segment HERE, through a pointer the compiler cannot trace back to it: left alone it
                    // loads them once, ahead of the walk, and the walk then carries (or spills to vector-register lanes) some
                    // forty scalar registers it never reads.
                    // (Where refills are whole tiles - primary rays, a wave refills a few times per frame - or the kernel sits at
                    // the register budget; the single-level AO pass refills whenever sixteen lanes idle and would wait on
                    // these loads thirty times as often: +5 % measured, profiles/r04_ab_procs.log.)
                    constexpr bool kReload = MODE == kModePrimary || MODE == kModeFused || TLAS;
                    const TraceParams &R = kReload ? *refill_params() : P;
                    // whole-tile refills only when frames are batched, so the frame is wave-uniform
                    uint32_t local_tile = my_tile, frame_base = 0u, vf = 0u, seed = R.frame;
                    if (MODE == kModeAo) {
                        // an AO batch shares its view and its primary hits; the lanes of a wave may hold different seeds
                        // (mid-tile refills stay on), so nothing here is wave-uniform
                        if (R.n_frames > 1u) {
                            frame_base = my_vf * R.frame_stride;
                            seed += my_vf;
                        }
                    } else if (R.n_frames > 1u) {
                        vf = __builtin_amdgcn_readfirstlane(div_uniform(my_tile, R.tiles_per_frame, R.rcp_tiles_per_frame));
                        local_tile = my_tile - vf * R.tiles_per_frame;
                        frame_base = vf * R.frame_stride;
                    }
                    const ViewDev &view = R.views[vf];
                    uint32_t px, py;
                    if (conv) {
                        // the pixel this lane's primary ray belonged to, back from its record index
                        if (R.compact) {
                            const uint32_t tile = (out_index >> 6) * R.shard_count + R.shard_index, k = out_index & 63u;
                            const uint32_t ty = div_uniform(tile, R.tiles_x, R.rcp_tiles_x);
                            px = (tile - ty * R.tiles_x) * 8u + (k & 7u);
                            py = ty * 8u + (k >> 3);
                        } else {
                            py = div_uniform(out_index, R.width, R.rcp_width);
                            px = out_index - py * R.width;
                        }
                    } else {
                        const uint32_t tile = local_tile * R.shard_count + R.shard_index;
                        const uint32_t k = item & 63u;
                        const uint32_t ty = div_uniform(tile, R.tiles_x, R.rcp_tiles_x);
                        px = (tile - ty * R.tiles_x) * 8u + (k & 7u);
                        py = ty * 8u + (k >> 3);
                        if (px < R.width && py < R.height) out_index = frame_base + (R.compact ? local_tile * 64u + k : py * R.width + px);
                    }
                    if (px < R.width && py < R.height) {
                        primary_dir(view, R.width, R.height, px, py, dx, dy, dz);
                        if (MODE == kModePrimary || (kFused && !conv)) {
                            r.ox = view.eye[0]; r.oy = view.eye[1]; r.oz = view.eye[2];
                            if (kFused) is_ao = false;
                            ok = true;
                        } else {
                            trx_hit ph;
                            if (kFused) { // the primary hit is still in this lane's registers
                                ph.t = t;
                                ph.prim = prim;
                                is_ao = true;
                            } else {
                                ph = R.primary[out_index - frame_base];
                            }
                            // a caller's record: whatever fails kernels.h's surface_record is a miss, no address is formed from it
                            // (a fused frame's record is its own walk's: a hit's prim comes from node bytes that were validated)
                            if (kFused ? ph.t < TRX_F32_MAX && ph.prim != TRX_INVALID : surface_record(ph, R.n_tris)) {
                                // normal of the hit triangle, flipped toward the viewer
                                const float4 *tp = P.tris + (size_t)ph.prim * 3;
                                float nx = tp[0].w, ny = tp[1].w, nz = tp[2].w; // cross(e1, e2)
                                if constexpr (TLAS) {
                                    if (R.inst_xform) {
                                        // object-space normal -> world: transpose of world-to-object
                                        const uint32_t pi = kFused ? hit_inst : R.primary_inst[out_index - frame_base];
                                        // (n_inst: behind TraceParams in the two-level kernels' block, which R is here)
                                        if (instance_row(pi, static_cast<const TraceParamsTlas &>(R).n_inst)) {
                                            const float4 *m = R.inst_xform + (size_t)pi * 3;
                                            const float3 w = normal_to_world(m[0], m[1], m[2], nx, ny, nz);
                                            nx = w.x; ny = w.y; nz = w.z;
                                        }
                                    }
                                }
                                TRX_AO_RAY(nx, ny, nz, dx, dy, dz, ph.t, view.eye, R.ao_eps, px, py, seed, r.ox, r.oy, r.oz)
                                ok = true;
                            } else if (!kFused) { // (a fused frame writes its AO misses where the primary ray ends)
                                trx_hit miss;
                                miss.t = __builtin_inff();
                                miss.prim = TRX_INVALID;
                                P.out[out_index] = miss;
                                if (TLAS && P.out_inst) P.out_inst[out_index] = TRX_INVALID;
                                if constexpr (COUNT)
                                    if (ray_cost) ray_cost[out_index] = trx_ray_cost{0u, 0u}; // (no ray: nothing visited)
                            }
                        }
                        if (MODE != kModeRays) {
                            r.tmin = 0.0f;
                            t = TRX_F32_MAX;
                        }
                    }
                }
                if (kFused) pend = false;
                if (ok) {
                    finish_ray_dir<(NODE & 1) == 0>(r, dx, dy, dz);
                    TRX_PUBLISH_RAY();
                    prim = TRX_INVALID;
                    sp = 0;
                    steps = trip; // the wave trip this ray starts at
                    if constexpr (COUNT) {
                        r_node = c_node;
                        r_tri = c_tri;
                    }
                    overflow = 0u;
                    cur = make_uint2(0u, 0x80000000u);
                    if (TLAS) {
                        tlas_sp = TRX_INVALID;
                        bvh_off = P.tlas_start;
                        cur_inst = hit_inst = TRX_INVALID;
                        if (P.inst_xform) { // (what the walk comes back to when it leaves a BLAS: kept in the wave's HBM area)
                            wray[0 * kWave + lane] = r.ox; wray[1 * kWave + lane] = r.oy; wray[2 * kWave + lane] = r.oz;
                            wray[3 * kWave + lane] = dx; wray[4 * kWave + lane] = dy; wray[5 * kWave + lane] = dz;
                        }
                    }
                    has_ray = true;
                }
            }
            if constexpr (kCull) {
                if (given != 0u) { // (wave-uniform) the wave's set of rays changed: the bounds of their 1/d, per axis
                    const unsigned long long have = __ballot(has_ray);
                    cull_ok = false;
                    if (have != 0ull && !(TLAS && P.inst_xform)) {
                        const int first = (int)__ffsll((long long)have) - 1;
                        const float ox0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(r.ox), first));
                        const float oy0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(r.oy), first));
                        const float oz0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(r.oz), first));
                        const uint32_t oct0 = (uint32_t)__builtin_amdgcn_readlane((int)r.oct_inv4, first) & 0xffu;
                        // magnitudes: with one sign per axis the order of |1/d| is the order of its bits
                        const uint32_t mx = __float_as_uint(r.ix) & 0x7fffffffu, my = __float_as_uint(r.iy) & 0x7fffffffu, mz = __float_as_uint(r.iz) & 0x7fffffffu;
                        const bool fits = !has_ray || (__float_as_uint(r.ox) == __float_as_uint(ox0) && __float_as_uint(r.oy) == __float_as_uint(oy0) &&
                                                       __float_as_uint(r.oz) == __float_as_uint(oz0) && (r.oct_inv4 & 0xffu) == oct0 &&
                                                       mx < 0x7f800000u && my < 0x7f800000u && mz < 0x7f800000u);
                        if (__ballot(!fits) == 0ull) {
                            const uint32_t a = lane >> 4; // this lane's axis as a decode lane (lanes 48..63: unused)
                            // (every lane contributes the magnitudes of ITS ray on all three axes: three max scans and three of the complement)
                            const uint32_t hx = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? mx : 0u), 63);
                            const uint32_t hy = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? my : 0u), 63);
                            const uint32_t hz = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? mz : 0u), 63);
                            const uint32_t lx = ~(uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? ~mx : 0u), 63);
                            const uint32_t ly = ~(uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? ~my : 0u), 63);
                            const uint32_t lz = ~(uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(has_ray ? ~mz : 0u), 63);
                            const uint32_t big = a == 0u ? hx : a == 1u ? hy : hz, small = a == 0u ? lx : a == 1u ? ly : lz;
                            // oct bits 2, 1, 0 (x, y, z) are SET for a non-negative direction (finish_ray_dir)
                            const bool neg = ((oct0 >> (2u - min(a, 2u))) & 1u) == 0u;
                            if ((lane & 15u) == 0u && a < 3u)
                                lds_cull_rays[a] = make_float4(__uint_as_float(neg ? (big | 0x80000000u) : small),
                                                               __uint_as_float(neg ? (small | 0x80000000u) : big),
                                                               a == 0u ? ox0 : a == 1u ? oy0 : oz0, 0.0f);
                            cull_ok = true;
                        }
                    }
                }
            }
        }
