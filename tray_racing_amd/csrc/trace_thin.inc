// trace_thin.inc - part of k_trace (kernels.hip), included as text inside the kernel: thin waves - eight lanes to a ray once a dry wave holds a handful
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
    // Thin waves.  An incoherent pass ends when its longest rays do (two thirds of a hairball-class AO pass is its
    // drain), and at the end those rays sit one or two to a wave: the wave then issues alone on its SIMD, one
    // instruction every four to five cycles whatever the instruction is, so a ray's trip costs its INSTRUCTION COUNT -
    // 213 vector instructions for the node test of one lane while 63 lanes idle.  So once a dry wave is down to 8 rays
    // they are moved to lanes 0, 8, 16 ... and every ray gets L = 8 lanes (four and two lanes to a ray from 16 and 32 rays
    // on were built and measured as well: the earlier steps cost what they gain, profiles/r04_thin_waves.log,
    // r04_ab_procs_11_thin_levels.log): lane j of a group tests child j of the node (its plane bytes,
    // loaded by address; the same IEEE operations as the per-lane test: node_children_intersect),
    // the contributions are ORed on the DPP network, and a leaf's triangles are tested L at a time and folded
    // into the ray's 64-bit {t, sequence} key with the same LDS atomic min as the cooperative rounds - node order,
    // triangle order, tie rule and every t are those of the one-lane walk (tested bit for bit).  A trip is about a
    // third of the instructions.  The walk is the plain one, rotated like the pipelined one: triangles of the node
    // tested last, then the next node.
    // (wave-uniform) may this wave go thin now?  Queues dry, a handful of rays, every stack inside its LDS part, no
    // hand-over with the other wave of the workgroup pending, no lane of a fused frame waiting to become an AO ray.
    auto thin_now = [&](uint32_t alive) -> bool {
        // (never more rays than the walk can hold, whatever the launch parameter says)
        constexpr uint32_t kHold = 8u;
        return exhausted && alive != 0u && alive <= (P.thin_max < kHold ? P.thin_max : kHold) && !(kMerge && merge_open) &&
               __ballot(has_ray && sp > (uint32_t)kLdsStack) == 0ull && !(kFused && __ballot(pend) != 0ull);
    };
    auto thin_walk = [&]() {
        constexpr uint32_t L = 8u; // lanes to a ray: one to a child of a node
        const uint32_t sub = lane & (L - 1u), first = lane & ~(L - 1u);
        {   // ---- move ray k (in lane order) to lane L k, stack column and all; give its L - 1 helpers the ray
            const unsigned long long act = __ballot(has_ray);
            // (diagnostic builds, tools/gpu_timeline_ao.py: when the wave first went thin, with how many rays, after how many trips)
            if (kTailDiag && diag_t0 == 0ull) {
                diag_t0 = wall_clock64();
                diag_chunk = (unsigned long long)__popcll(act);
                diag_tiles = trip;
            }
            // the k-th ray's lane, through a table in LDS (the cooperative rounds' run-head table, idle here)
            if (has_ray) lds_head[lane_rank(act)] = lane;
            __builtin_amdgcn_wave_barrier();
            const bool filled = lane / L < (uint32_t)__popcll(act);
            const int src = filled ? (int)lds_head[lane / L] : (int)lane;
            __builtin_amdgcn_wave_barrier();
            const bool owner = filled && sub == 0u;
            r.ox = __shfl(r.ox, src); r.oy = __shfl(r.oy, src); r.oz = __shfl(r.oz, src);
            r.dx = __shfl(r.dx, src); r.dy = __shfl(r.dy, src); r.dz = __shfl(r.dz, src);
            r.ix = __shfl(r.ix, src); r.iy = __shfl(r.iy, src); r.iz = __shfl(r.iz, src);
            r.tmin = __shfl(r.tmin, src);
            r.oct_inv4 = (uint32_t)__shfl((int)r.oct_inv4, src);
            t = __shfl(t, src);
            prim = (uint32_t)__shfl((int)prim, src);
            out_index = (uint32_t)__shfl((int)out_index, src);
            const uint32_t age = (uint32_t)__shfl((int)(trip - steps), src);
            steps = trip - age;
            cur.x = (uint32_t)__shfl((int)cur.x, src); cur.y = (uint32_t)__shfl((int)cur.y, src);
            ptri.x = (uint32_t)__shfl((int)ptri.x, src); ptri.y = (uint32_t)__shfl((int)ptri.y, src);
            overflow = (uint32_t)__shfl((int)overflow, src);
            if (kFused) is_ao = __shfl(is_ao ? 1 : 0, src) != 0;
            const uint32_t sp_src = (uint32_t)__shfl((int)sp, src);
            uint32_t sp_max = owner ? sp_src : 0u;
            for (int off = 32; off > 0; off >>= 1) sp_max = max(sp_max, (uint32_t)__shfl_xor((int)sp_max, off));
            // (the destination address is formed HERE: left alone the compiler forms it at kernel start and the one-launch
            // frame, at the register budget, spills it)
            uint32_t dst = lane;
            asm volatile("" : "+v"(dst));
            for (uint32_t k = 0; k < sp_max; k++) { // (entries beyond a ray's own top are copied too: harmless)
                const uint2 e = lds_ld(&lds_stack[k * kWave + (uint32_t)src]);
                __builtin_amdgcn_wave_barrier();
                if (owner) lds_st(&lds_stack[k * kWave + dst], e);
                __builtin_amdgcn_wave_barrier();
            }
            sp = owner ? sp_src : 0u;
            has_ray = owner;
            if (!owner) {
                ptri = make_uint2(0u, 0u);
                cur = make_uint2(0u, 0u);
                if (!filled) r.oct_inv4 &= 0x3fffffffu; // (a group without a ray must not veto the literal-division shortcuts)
            }
            if (owner) TRX_PUBLISH_RAY();
            fetched = false;
            __builtin_amdgcn_s_setprio(3);
        }
        unsigned long long *const lds_key = reinterpret_cast<unsigned long long *>(lds_res);
        // The trip is rotated like the pipelined walk's, and one step further: (1) the ray's next node is chosen and its
        // bytes are requested, (2) the triangles of the node tested in the PREVIOUS trip are tested - the first L
        // records were requested at the end of that trip - (3) a ray with no node left is finished, (4) the requested node
        // is tested with the t those triangles left, (5) the first L triangle records of the new leaf hits are
        // requested.  A thin wave's time is its rays' dependent round trips to memory.  (The requests are plain loads: an
        // `asm volatile` barrier naming the loaded registers right behind them - there until late in round 4 "to keep
        // the loads early" - makes the compiler wait for them on the spot; without it the AO pass of a hairball-class
        // scene runs 6 % faster, random rays 6-7 %.  Requesting (5) right behind (1) instead, both in flight together
        // and nothing across the back-edge, was built as well and measures the same to slightly slower.)
        uint4 n0 = make_uint4(0u, 0u, 0u, 0u), n1 = n0;
        uint32_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u, q4 = 0u, q5 = 0u;
        float4 ta = unspecified4(), tb = unspecified4(), tc = unspecified4();
        uint32_t gx = 0u, gy = 0u, cnt = 0u, pre_local = 0u;
        // (the records of all entered children touched the moment their parent is tested: measured slower, profiles/r06_ray_service.log)
        // (the one-launch frame comes back from here into its loop, whose registers stay live meanwhile: it does without
        // the early triangle request, twelve registers carried from trip to trip)
        constexpr bool kPre = !kFused;
        // (the ray service's first triangle records requested behind the next node's bytes instead: measured slower,
        // profiles/r06_ray_service.log)
        auto request_triangles = [&]() { // (5): the group's pending triangle group, and this lane's record of its first L
            cnt = 0u;
            if (__ballot(ptri.y != 0u) == 0ull) return; // (most trips of a handful of rays find no leaf)
            gx = group_first(ptri.x);
            gy = group_first(ptri.y);
            cnt = (uint32_t)__popc(gy);
            if (kPre && sub < cnt) {
                pre_local = select_from_top(gy, sub); // (kept for (2): the search is thirty-five instructions of a lone wave's trip)
                const float4 *tp = P.tris + (size_t)(gx + pre_local) * 3;
                ta = tp[0];
                tb = tp[1];
                tc = tp[2];
            }
        };
        request_triangles(); // (a wave that comes from the pipelined walk brings pending triangle groups)
        // wave-uniform: what is in flight is finished, then out - a fused frame's primary ray has hit
        bool leaving = false;
        // Two-level scenes (the ray service only): the group's world-space ray, to come back to when a BLAS is left and to
        // transform into the next instance's space (trace_walk_plain.inc keeps it in the wave's HBM area; here the eight
        // lanes of a group all hold the ray, so the copy is six registers of each).  The walk itself follows
        // trace_walk_plain.inc's two-level steps - query_tlas.hlsl:410-446, 480-486 - rotated like everything else here.
        // (only the service calls it over two-level scenes: the passes' kThin is false there, trace_state.inc - a ray that comes in
        // through the move above would need its world-space copy and its two-level state moved as well)
        float wox = 0.0f, woy = 0.0f, woz = 0.0f, wdx = 0.0f, wdy = 0.0f, wdz = 0.0f;
#ifdef TRX_SVC_PHASES   // (tuning builds: shader-clock cycles per step of the service walker's trip, printed when the service stops)
        uint32_t ph[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        unsigned long long ph_t = __builtin_readcyclecounter();
#define SVC_MARK(k) do { if constexpr (MODE == kModeService) { const unsigned long long now_ = __builtin_readcyclecounter(); ph[k] += (uint32_t)(now_ - ph_t); ph_t = now_; } } while (0)
#else
#define SVC_MARK(k) do { } while (0)
#endif
        for (;;) {
            trip++;
            if constexpr (MODE == kModeService) {
                // ---- (0) the ray service: a group without a ray looks into its mailbox (kernels.h, kSvcRays)
                const uint32_t g = lane >> 3;
                const bool gfree = g < kSvcRays && ((__ballot(has_ray) >> first) & 1ull) == 0ull; // (the upper groups have no slots)
                uint32_t in_seq = svc_seq;
                if (gfree) in_seq = svc_box[16u * g + 12u];
                const bool fresh = gfree && in_seq != svc_seq; // (the same in all eight lanes of a group)
                if (__ballot(fresh) != 0ull) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if (fresh) {
                        const svc_word *q = svc_box + 16u * g;
                        r.ox = __uint_as_float(q[0]); r.oy = __uint_as_float(q[1]); r.oz = __uint_as_float(q[2]);
                        const float dx = __uint_as_float(q[3]), dy = __uint_as_float(q[4]), dz = __uint_as_float(q[5]);
                        r.tmin = __uint_as_float(q[6]);
                        t = fminf(__uint_as_float(q[7]), TRX_F32_MAX);
                        finish_ray_dir<(NODE & 1) == 0>(r, dx, dy, dz);
                        if constexpr (TLAS) {
                            wox = r.ox; woy = r.oy; woz = r.oz;
                            wdx = dx; wdy = dy; wdz = dz;
                            tlas_sp = TRX_INVALID;
                            bvh_off = P.tlas_start;
                            cur_inst = hit_inst = TRX_INVALID;
                        }
                        svc_seq = in_seq;
                        svc_t0 = wall_clock64();
                        prim = TRX_INVALID;
                        sp = 0u;
                        steps = trip;
                        overflow = 0u;
                        ptri = make_uint2(0u, 0u);
                        has_ray = sub == 0u;
                        cur = has_ray ? make_uint2(0u, 0x80000000u) : make_uint2(0u, 0u);
                    }
                }
                if (__ballot(has_ray) == 0ull) { // nothing to step: leave when told to, else look again shortly
                    if (svc_box[192] != 0u) break;
                    __builtin_amdgcn_s_sleep(4);
#ifdef TRX_SVC_PHASES
                    ph_t = __builtin_readcyclecounter();
#endif
                    continue;
                }
#ifdef TRX_SVC_PHASES
                ph[7]++;
#endif
            }
            SVC_MARK(0);
            // ---- (1) the next node of every ray that holds a node group; its bytes are requested
            const bool had_group = has_ray && (cur.y & 0xff000000u) != 0u;
            const bool stepping = had_group && !leaving;
            uint32_t node_index = 0u;
            if (stepping) {
                const uint32_t hits_imask = cur.y;
                const uint32_t child_bit = 31u - (uint32_t)__builtin_clz(hits_imask);
                cur.y &= ~(1u << child_bit);
                const uint32_t slot = (child_bit - 24u) ^ (r.oct_inv4 & 0xffu);
                node_index = cur.x + (uint32_t)__popc(hits_imask & ~(0xffffffffu << slot));
                if (TLAS) node_index += bvh_off;
                stack_push(cur, (cur.y & 0xff000000u) != 0u);
            }
            const bool gstep = ((__ballot(stepping) >> first) & 1ull) != 0ull;
            if (gstep) {
                const uint4 *np = P.nodes + (size_t)group_first(node_index) * 5;
                const uint8_t *nb = reinterpret_cast<const uint8_t *>(np) + sub;
                n0 = np[0];
                n1 = np[1];
                // the plane bytes of this lane's child by address: min planes at +32 / +48 / +64, max planes eight bytes
                // on; near = max where d < 0
                const uint32_t xn = r.dx < 0.0f ? 8u : 0u, yn = r.dy < 0.0f ? 8u : 0u, zn = r.dz < 0.0f ? 8u : 0u;
                const uint8_t *const bx = nb + 32u, *const by = nb + 48u, *const bz = nb + 64u;
                q0 = bx[xn]; q1 = bx[xn ^ 8u];
                q2 = by[yn]; q3 = by[yn ^ 8u];
                q4 = bz[zn]; q5 = bz[zn ^ 8u];
            }
            SVC_MARK(1);
            // ---- (2) triangles of the node tested in the previous trip, L at a time; the first L are here already
            if (__ballot(cnt != 0u) != 0ull) {
                const uint32_t init_lo = tie_first ? 0u : 0xffu;
                if (sub == 0u) lds_res[lane] = make_uint2(init_lo, ordered_bits(t + 0.0f));
                __builtin_amdgcn_wave_barrier();
                auto test_one = [&](uint32_t local, const float4 &a, const float4 &b, const float4 &c) {
                    float tt = TRX_F32_MAX; // the tie test against the ray's t is the atomic min (see the cooperative rounds)
                    if (intersect_tri(r, a, b, c, tt, false)) {
                        const uint32_t neg_zero = __float_as_uint(tt) == 0x80000000u ? 1u : 0u;
                        const uint32_t lo = ((tie_first ? 31u - local : local) << 1) | neg_zero;
                        atomicMin(&lds_key[first], ((unsigned long long)ordered_bits(tt + 0.0f) << 32) | lo);
                    }
                };
                // (the first L stand apart from the loop: a loop that loads waits at its head for everything in flight -
                // the node bytes requested in (1) included - where these only need their own records)
                uint32_t j = sub;
                if (kPre) {
                    if (j < cnt) test_one(pre_local, ta, tb, tc);
                    j += L;
                }
                for (; __ballot(j < cnt) != 0ull; j += L) {
                    if (j < cnt) {
                        const uint32_t local = select_from_top(gy, j);
                        const float4 *tp = P.tris + (size_t)(gx + local) * 3;
                        const float4 a = tp[0], b = tp[1], c = tp[2];
                        test_one(local, a, b, c);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (sub == 0u && cnt != 0u) {
                    const uint2 won = lds_res[lane];
                    if (won.x != init_lo) {
                        const uint32_t local = tie_first ? 31u - (won.x >> 1) : (won.x >> 1);
                        t = (won.x & 1u) ? -0.0f : __uint_as_float(unordered_bits(won.y));
                        prim = ptri.x + local;
                        if (TLAS) hit_inst = cur_inst;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            SVC_MARK(2);
            ptri = make_uint2(0u, 0u);
            // ---- (3) the end of a ray: it had no node left to visit and its last triangles are in
            if (has_ray) {
                // (two-level walks: a ray may stand without a node group for a trip while its last triangles of a BLAS are
                // tested - the way back to the TLAS is taken behind them, see step (4))
                bool done = !had_group && (!TLAS || sp == 0u);
                if (MODE == kModeRays && P.any_hit != 0u && prim != TRX_INVALID) done = true; // (a node in flight is simply not looked at)
                if (__builtin_expect((trip & 1023u) == 0u, 0)) { // step cap: every wave reaches an exit
                    if (trip - steps > kMaxSteps) {
                        overflow = 1u;
                        done = true;
                    }
                }
                if (done) finish_lane();
            }
            SVC_MARK(3);
            if (MODE != kModeService && __ballot(has_ray) == 0ull) break; // (the ray service stays: its groups take new rays at (0))
            // (fused frames: a primary ray has hit and waits to become an AO ray at the refill point.  What is in flight is
            // finished first - this trip's node tests, then, in one more trip that chooses no node, their triangles - so
            // that every ray left holds a node group and nothing pending: the state the other walks expect.)
            if (leaving) break;
            const unsigned long long alive_mask = __ballot(has_ray);
            if (kFused && __ballot(pend) != 0ull) leaving = true;
            // ---- (4) node test, a child per lane, for the rays still there
            const bool galive = ((alive_mask >> first) & 1ull) != 0ull;
            const float gt = __uint_as_float(group_first(__float_as_uint(t)));
            const int pow2 = (NODE & 1) ? 0 : pow2_exact(P, r, gstep && galive);
            uint32_t contrib = 0u;
            if (gstep && galive) {
                const uint32_t meta = (sub < 4u ? n1.z : n1.w) >> (8u * (sub & 3u));
                const uint32_t q[6] = {q0, q1, q2, q3, q4, q5};
                contrib = node_children_intersect<NODE, 1>(r, gt, n0, meta, q, pow2);
            }
            const uint32_t hitmask = group_or_to_first(contrib);
            if (stepping && has_ray) {
                cur.x = n1.x;
                ptri.x = n1.y;
                cur.y = (hitmask & 0xff000000u) | (n0.w >> 24);
                ptri.y = hitmask & 0x00ffffffu;
                if constexpr (!TLAS) {
                    if ((cur.y & 0xff000000u) == 0u && sp != 0u) {
                        cur = stack_pop();
                        if (__builtin_expect(overflow != 0u, 0)) cur = make_uint2(0u, 0u); // past the last entry: finish
                    }
                }
            }
            if constexpr (TLAS) {
                // The owner lane decides; what it decides about the RAY (back to world space / into instance gidx) goes to
                // the group's eight lanes as one word: bit 0 = restore, bit 1 = enter, bits 2.. = the instance.
                uint32_t word = 0u;
                if (has_ray) {
                    // the leaf hits of a TLAS node are instances (query_tlas.hlsl:410-446): enter the nearest one's BLAS
                    bool enter = stepping && tlas_sp == TRX_INVALID && ptri.y != 0u;
                    uint2 grp = ptri;
                    if (!enter && (cur.y & 0xff000000u) == 0u && sp != 0u) {
                        const bool crossing = sp == tlas_sp;
                        // (the BLAS's last triangles are tested in the NEXT trip, with the BLAS's ray: the way back waits for them)
                        if (!(crossing && ptri.y != 0u)) {
                            if (crossing) { // back to the TLAS (query_tlas.hlsl:480-486)
                                tlas_sp = TRX_INVALID;
                                bvh_off = P.tlas_start;
                                cur_inst = TRX_INVALID;
                                word = 1u;
                            }
                            cur = stack_pop();
                            if (__builtin_expect(overflow != 0u, 0)) cur = make_uint2(0u, 0u); // past the last entry: finish
                            if ((cur.y & 0xff000000u) == 0u && cur.y != 0u) { // a parked group of instances
                                grp = cur;
                                cur = make_uint2(0u, 0u);
                                enter = true;
                            }
                        }
                    }
                    if (enter) {
                        const uint32_t local = 31u - (uint32_t)__clz((int)grp.y);
                        grp.y &= ~(1u << local);
                        const uint32_t gidx = grp.x + local;
                        stack_push(grp, grp.y != 0u);
                        stack_push(cur, (cur.y & 0xff000000u) != 0u);
                        tlas_sp = sp;
                        bvh_off = P.inst[gidx];
                        cur_inst = gidx;
                        // the walk of the BLAS starts at its node 0 - or at the subtree a re-braided TLAS primitive stands for
                        cur = make_uint2(P.inst_entry ? P.inst_entry[gidx] : 0u, 0x80000000u);
                        ptri = make_uint2(0u, 0u);
                        word = 2u | (gidx << 2);
                    }
                }
                if (P.inst_xform) {
                    word = group_first(word);
                    if (word & 2u) {
                        // the ray in the instance's object space
                        const float4 *m = P.inst_xform + (size_t)(word >> 2) * 3;
                        const float4 r0 = m[0], r1 = m[1], r2 = m[2];
                        TRX_RAY_TO_OBJECT(r0, r1, r2, wox, woy, woz, wdx, wdy, wdz, r.ox, r.oy, r.oz, odx, ody, odz)
                        finish_ray_dir<(NODE & 1) == 0>(r, odx, ody, odz);
                    } else if (word & 1u) { // "Reset Ray to untransformed version" (query_tlas.hlsl:484)
                        r.ox = wox; r.oy = woy; r.oz = woz;
                        finish_ray_dir<(NODE & 1) == 0>(r, wdx, wdy, wdz);
                    }
                }
            }
            SVC_MARK(4);
            // ---- (5)
            request_triangles();
            SVC_MARK(5);
        }
#ifdef TRX_SVC_PHASES
        if constexpr (MODE == kModeService) {
            if (lane < 8u) P.svc_ring[(size_t)(blockIdx.x * kSvcRays) * kSvcSlotWords + 24u + lane] = ph[lane];
        }
#endif
#undef SVC_MARK
        __builtin_amdgcn_s_setprio(0);
        if (PIPE) { // (no node was in flight all the while: tell the register allocator so, it cannot see through `fetched`)
            const float4 u0 = unspecified4(), u1 = unspecified4(), u2 = unspecified4(), u3 = unspecified4(), u4 = unspecified4();
            pn0 = make_uint4(__float_as_uint(u0.x), __float_as_uint(u0.y), __float_as_uint(u0.z), __float_as_uint(u0.w));
            pn1 = make_uint4(__float_as_uint(u1.x), __float_as_uint(u1.y), __float_as_uint(u1.z), __float_as_uint(u1.w));
            pn2 = make_uint4(__float_as_uint(u2.x), __float_as_uint(u2.y), __float_as_uint(u2.z), __float_as_uint(u2.w));
            pn3 = make_uint4(__float_as_uint(u3.x), __float_as_uint(u3.y), __float_as_uint(u3.z), __float_as_uint(u3.w));
            pn4 = make_uint4(__float_as_uint(u4.x), __float_as_uint(u4.y), __float_as_uint(u4.z), __float_as_uint(u4.w));
        }
    };
    // The thin walk of a dry wave; returns with no ray left or, fused frames, with a lane waiting to become an AO ray.
    auto thin_all = [&]() {
        if (!(kFused && __ballot(pend) != 0ull) && __ballot(has_ray) != 0ull) thin_walk();
    };
