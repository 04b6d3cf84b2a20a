// trace_triangles.inc - part of k_trace (kernels.hip), included as text inside the kernel: the triangle phase of a node step (per-lane rounds, cooperative rounds)
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
        // ---- traverse ------------------------------------------------------------
        // The loop is wave-uniform (every lane iterates, work is predicated on `act`), so that the
        // triangle phase can use all 64 lanes whichever lanes own the triangles.
        const uint32_t keep = kWave - refill_idle; // leave when this few lanes remain
        // ---- triangle phase ---------------------------------------------------------
            // Each lane owns cnt triangle tests (the hit leaves of its node, highest bit first).
            // Few per lane: every owner tests its own, one round per triangle.  Otherwise the
            // wave's (ray, triangle) pairs are laid out densely over all 64 lanes: pair g goes to
            // lane g % 64, tests read the owner's ray from LDS, and owners then commit their
            // results in order, so a ray's triangle sequence (and its tie rule) is unchanged.
        auto triangle_phase = [&](uint2 tri) {
            const uint32_t cnt = (uint32_t)__popc(tri.y);
            if (__ballot(cnt != 0u) != 0ull) {
                if (COUNT) {
                    uint32_t mx = cnt, sum = cnt;
                    for (int off = 32; off > 0; off >>= 1) {
                        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
                        sum += (uint32_t)__shfl_xor((int)sum, off);
                    }
                    if (lane == 0) {
                        atomicAdd(&P.ctr->hist_max[min(mx, 15u)], 1u);
                        if (!kTune || !(P.tune & 0x100u)) atomicAdd(&P.ctr->hist_total[min((sum + 7u) >> 3, 15u)], 1u);
                    }
                }
                // Cooperative rounds cost about three per-lane rounds of VALU work (scans, owner look-up, the LDS
                // hand-offs), so they only pay when the wave's triangles sit in few lanes: 64 coherent rays testing
                // the same two triangles are 128 pairs = 2 cooperative rounds, but also just 2 per-lane rounds.
                bool coop = false;
                uint32_t incl = 0u, total = 0u, mx = 1u;
                if (__ballot(cnt >= P.tri_compact_min) != 0ull) {
                    incl = wave_scan_add(cnt);
                    total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    mx = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(cnt), 63);
                    // per-lane rounds carry kBatch triangles of a lane each, cooperative rounds 64 pairs of the wave
                    coop = (mx + (uint32_t)kBatch - 1u) / (uint32_t)kBatch > P.tri_coop_ratio * ((total + 63u) >> 6);
                }
                if (!coop) {
                    // Per-lane rounds, up to kBatch triangles of a lane per round: their records are requested
                    // together (one memory round trip per round instead of one per triangle; on incoherent rays the
                    // triangle phase is 55-60 % of a trip and most of that is these round trips) and tested in the
                    // lane's own order, highest bit first, each against the t its predecessor left.
                    while (tri.y != 0u) {
                        uint32_t gidx[kBatch];
                        bool have[kBatch];
                        float4 ta[kBatch], tb[kBatch], tc[kBatch];
#pragma unroll
                        for (int k = 0; k < kBatch; k++) {
                            have[k] = tri.y != 0u;
                            const uint32_t local = 31u - (uint32_t)__builtin_clz(tri.y | 1u);
                            tri.y &= ~(1u << local);
                            gidx[k] = tri.x + local;
                            ta[k] = tb[k] = tc[k] = unspecified4(); // no lane without a triangle reads them
                            if (have[k]) {
                                const float4 *tp = P.tris + (size_t)gidx[k] * 3;
                                ta[k] = tp[0];
                                tb[k] = tp[1];
                                tc[k] = tp[2];
                            }
                        }
                        // keep the loads of a round together and ahead of the arithmetic: left alone the compiler
                        // sinks them behind the first determinant, serialising the memory latencies again
                        if constexpr (kBatch > 1)
#pragma unroll
                        for (int k = 0; k < kBatch; k++)
                            asm volatile("" : "+v"(ta[k].x), "+v"(ta[k].y), "+v"(ta[k].z), "+v"(ta[k].w), "+v"(tb[k].x), "+v"(tb[k].y), "+v"(tb[k].z), "+v"(tb[k].w), "+v"(tc[k].x), "+v"(tc[k].y), "+v"(tc[k].z), "+v"(tc[k].w));
#pragma unroll
                        for (int k = 0; k < kBatch; k++) {
                            if (have[k]) {
                                if (COUNT) {
                                    c_tri++;
                                    if (lane_rank(__ballot(1)) == 0) c_wtri++;
                                    if (P.touch_tris) P.touch_tris[gidx[k]] = 1;
                                }
                                if (intersect_tri<true>(r, ta[k], tb[k], tc[k], t, tie_first)) {
                                    prim = gidx[k];
                                    if (TLAS) hit_inst = cur_inst;
                                }
                            }
                        }
                    }
                } else {
                    // Cooperative rounds: the wave's (ray, triangle) pairs laid out densely, pair g on lane g % 64.  The
                    // tester finds its owner (a max-scan over the run heads), picks the owner's j-th triangle, tests it
                    // against the owner's ray and folds the result into the owner's 64-bit key with ONE LDS atomic min:
                    // key = {order-preserving image of t, tie word}.  The owner's key starts as its current t with a tie
                    // word that wins (TIE_FIRST: tt < t commits) or loses (tt <= t commits) every tie, and a pair's
                    // tie word is its place in the owner's own sequence (highest bit first), so the minimum IS the
                    // result of the sequential loop "for each triangle in order: if closer, commit": no per-owner
                    // commit loop, no result table, one barrier-free pass per window.
                    const uint32_t excl = incl - cnt;
                    lds_grp[lane] = tri;
                    lds_pref[lane] = excl;
                    const uint32_t init_lo = tie_first ? 0u : 0xffu;
                    unsigned long long *const lds_key = reinterpret_cast<unsigned long long *>(lds_res);
                    lds_res[lane] = make_uint2(init_lo, ordered_bits(t + 0.0f));
                    if (COUNT) c_tri += cnt;
                    for (uint32_t base = 0; base < total; base += kWave) {
                        // owner of every pair of this window: heads mark where each owner's run starts
                        // (the table is cleared for every window; tagging the heads with a window number instead, so
                        // that stale ones lose the max-scan and the clearing store goes, measured -1 % on one pass
                        // and was not kept)
                        lds_head[lane] = 0u;
                        __builtin_amdgcn_wave_barrier();
                        const uint32_t run_begin = max(excl, base), run_end = min(excl + cnt, base + kWave);
                        if (run_begin < run_end) lds_head[run_begin - base] = lane + 1u;
                        __builtin_amdgcn_wave_barrier();
                        const uint32_t owner1 = wave_scan_max(lds_head[lane]);
                        const uint32_t g = base + lane;
                        if (g < total) {
                            const uint32_t ol = (owner1 - 1u) & 63u; // (owner1 is 1..64; the mask keeps a corrupted table inside this wave's LDS)
                            const uint2 grp = lds_grp[ol];
                            const uint32_t local = select_from_top(grp.y, g - lds_pref[ol]);
                            const uint32_t gidx = grp.x + local;
                            if (COUNT && P.touch_tris) P.touch_tris[gidx] = 1;
                            const float4 *tp = P.tris + (size_t)gidx * 3;
                            float4 a = tp[0], b = tp[1], c4 = tp[2];
                            const float4 ro = lds_ray[2u * ol], rd = lds_ray[2u * ol + 1u];
                            asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w), "+v"(c4.x), "+v"(c4.y), "+v"(c4.z), "+v"(c4.w));
                            Ray orr;
                            orr.ox = ro.x; orr.oy = ro.y; orr.oz = ro.z; orr.tmin = ro.w;
                            orr.dx = rd.x; orr.dy = rd.y; orr.dz = rd.z;
                            float tt = TRX_F32_MAX; // the tie test against the owner's t is the atomic min
                            if (intersect_tri(orr, a, b, c4, tt, false)) {
                                // -0.0 and +0.0 are one value to the sequential compare: they share a key, and the
                                // tie word's lowest bit remembers which one the pair really produced
                                const uint32_t neg_zero = __float_as_uint(tt) == 0x80000000u ? 1u : 0u;
                                const uint32_t lo = ((tie_first ? 31u - local : local) << 1) | neg_zero;
                                const unsigned long long key = ((unsigned long long)ordered_bits(tt + 0.0f) << 32) | lo;
                                atomicMin(&lds_key[ol], key);
                            }
                        }
                        if (COUNT && lane == 0) c_wtri++;
                    }
                    __builtin_amdgcn_wave_barrier();
                    const uint2 won = lds_res[lane];
                    if (cnt != 0u && won.x != init_lo) { // some pair of this lane beat (or tied its way past) the current t
                        const uint32_t local = tie_first ? 31u - (won.x >> 1) : (won.x >> 1);
                        t = (won.x & 1u) ? -0.0f : __uint_as_float(unordered_bits(won.y));
                        prim = tri.x + local;
                        if (TLAS) hit_inst = cur_inst;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }

        };




