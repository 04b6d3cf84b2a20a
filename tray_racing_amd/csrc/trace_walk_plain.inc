// trace_walk_plain.inc - part of k_trace (kernels.hip), included as text inside the kernel: the plain walk (coherent primary rays, two-level scenes): fetch, test, triangles, pop
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
            // the walk goes on while more lanes hold a ray than this: `alive != 0 && (exhausted || alive > keep)` as ONE
            // comparison (nothing inside the walk changes `exhausted`; `keep` stays a runtime value)
            // (the two-level kernels have no scalar to spare across the loop - it would be one more parked in a vector lane -
            // and form the bound where they use it)
            const uint32_t leave_at = TLAS ? 0u : exhausted ? 0u : keep;
            for (;;) {
                const bool act = has_ray;
                const unsigned long long act_mask = ballot64(act); // (once per trip: for the look and for the end of the trip)
                const int pow2 = (NODE & 1) ? 0 : pow2_exact(P, r, act); // (literal-division variants only)
                uint2 tri = make_uint2(unspecified1(), 0u); // (.x: read where .y says there are triangles; no trip pays to zero it)
                trip++;
                if (!TLAS && MODE != kModePrimary && (trip & 7u) == 0u) old_ray_priority(); // (measured without effect in the two-level kernels)
                // Coherent primary rays (BLAS only): when every lane that steps visits the SAME node - 47 % of the wave-level
                // node steps on the bistro-class frame, 90 % on the kitchen-class one - its 48 quantised plane bytes are
                // converted once, one byte per lane, parked in LDS as floats and read back by address (node_intersect_kept)
                // (two-level walks too since round 5 - absolute node indices, lanes with a parked triangle group excluded: in round 4
                // the two-level primary kernel spilled with it (4K frame +4 %, profiles/r04_ab_procs_16); with the world-space ray
                // copies out of the registers (kernels.h, kWaveScratch) it has 121 and the 4K frame runs 3.3 % faster,
                // profiles/r05_ab_5_tlas.log)
                constexpr bool kUni = MODE == kModePrimary && !COUNT;
                uint32_t lane_step = 1u; // wave-uniform: 0 once the trip's step has been a uniform step
                // The node a lane steps to next, worked out ONCE per trip, for the look below and for either kind of step.
                // (two-level walks: a lane may hold a parked triangle group instead of a node group, and node
                // indices are absolute - rays inside different instances of one BLAS do share its nodes, each
                // with its own object-space ray.  BLAS-only: a lane at the top of the loop always holds a node group -
                // triangle groups are drained in the trip that found them; only the TLAS walk parks them on the stack.)
                // Lanes without a group leave both words unspecified: nothing reads them there.
                const bool group = act && (!TLAS || (cur.y & 0xff000000u) != 0u);
                uint32_t node_index = unspecified1(), child_bit = unspecified1();
                if (group) {
                    const uint32_t hits_imask = cur.y; // != 0
                    child_bit = 31u - (uint32_t)__builtin_clz(hits_imask);
                    const uint32_t slot = (child_bit - 24u) ^ (r.oct_inv4 & 0xffu);
                    node_index = cur.x + (uint32_t)__popc(hits_imask & ~(0xffffffffu << slot));
                    if (TLAS) node_index += bvh_off;
                }
                if constexpr (kUni) {
                    // (the look itself is some thirty instructions.  Before the packet test a trip whose lanes wanted different
                    // nodes was followed by kUniCool = 1 trips that did not look - bistro-class frame -0.5 %, hairball-class
                    // -0.8 %, kitchen-class -0.2 %, profiles/r05_ab_7_unicool.log; with it a uniform step is worth more than the
                    // look costs: looking every trip -0.8 % / +-0 / -0.9 %, two trips off +0.5 / -0.2 / +0.2 %, r05_ab_22_unicool.log.
                    // The two-level walk keeps its one trip off: 4K frame 2.775 against 2.789 ms, r05_ab_27_cool_tlas.log.
                    // The node's second quarter requested ahead of the packet test: +0.8 %, r05_ab_23_n1early.log.)
                    constexpr uint32_t kUniCool = TLAS ? 1u : 0u;
                    if (kUniCool != 0u && uni_cool != 0u) {
                        uni_cool--;
                    } else
                    if (P.uni_decode) {
                        // (`first` is a node of the scene whenever the step turns out uniform: the first stepping lane's, or
                        // node 0 in a trip in which no lane steps - a scalar select)
                        const unsigned long long stepping = act_mask;
                        uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)node_index, (int)(__ffsll((long long)stepping) - 1));
                        if (stepping == 0ull) first = 0u;
                        // (the lanes that differ as ONE comparison's mask, cut to the stepping lanes by the scalar unit: the
                        // ballot of `act && ...` went through a 0 / 1 register and a second comparison)
                        unsigned long long differ = ballot64(node_index != first);
                        if (TLAS) differ |= ~ballot64((cur.y & 0xff000000u) != 0u);
                        if ((differ & stepping) == 0ull) { // wave-uniform: every lane takes this branch or none does
                            const uint4 *np = P.nodes + (size_t)first * 5;
                            // 48 lanes convert one byte each (whether or not they hold a ray), LDS hands the floats to all
                            // (byte 32 + 8 p + c = plane p of child c, planes in the order min_x max_x min_y max_y min_z max_z; the
                            // second table lives in the triangle phase's window area, idle during a node step)
                            // Packet culling (kCull): the decode lanes also bound their plane's parameter over the wave's rays -
                            // near planes from below, far planes from above, with the per-ray test's own operations at the
                            // ends of the rays' 1/d interval (monotone: see node_intersect_kept) - and a child whose bounds
                            // exclude every ray is left out of the per-ray test for the whole wave.  (Two other shapes of
                            // this were built and measured slower, EXPERIMENTS 5.11: the kept children filed into the first
                            // table slots - one LDS round trip more - and the whole test in registers, DPP and v_readlane.)
                            const bool culling = kCull && cull_ok && ((NODE & 1) != 0 || pow2 == 2); // (literal divisions: where every ray of the step takes both shortcuts)
                            // (scalar-cache header reads: measured slower, profiles/r06_ab_uni_scalar.log)
                            // (every lane loads the record, with or without a ray - one line, broadcast: no access more than for
                            // the lanes that need it, and no zeroes for the others.  A variable of this trip only, DESIGN.md section 4.)
                            const uint4 n0 = np[0];
                            // (the lane number taken afresh here, not as loop-invariant masks: measured slower, profiles/r06_ab_lane_spills.log)
                            const uint32_t dl = lane;
                            if (dl < 48u) {
                                const float v = (float)reinterpret_cast<const uint8_t *>(np)[32u + dl];
                                const uint32_t a = dl >> 4, slot = a * 16u + (dl & 7u) * 2u, is_max = (dl >> 3) & 1u;
                                lds_dec[slot + is_max] = v;
                                lds_dec_neg[slot + (is_max ^ 1u)] = v;
                                if (culling) {
                                    const float4 cr = lds_cull_rays[a]; // {lo, hi} of the rays' 1/d on this dl's axis, their origin there
                                    const float pa = __uint_as_float(a == 0u ? n0.x : a == 1u ? n0.y : n0.z);
                                    const float ea = __uint_as_float(((n0.w >> (8u * a)) & 0xffu) << 23);
                                    const float c = pa - cr.z;
                                    const float alo = ea * cr.x, ahi = ea * cr.y;
                                    const float b0 = c * cr.x, b1 = c * cr.y;
                                    float blo = fminf(b0, b1), bhi = fmaxf(b0, b1);
                                    if ((NODE & 1) == 0) { // b = RN(c / d) there, within 3 x 2^-24 of RN(c RN(1/d)): the ends move out by 2^-21 of their magnitudes
                                        blo = __builtin_fmaf(-fabsf(blo), 0x1p-21f, blo);
                                        bhi = __builtin_fmaf(fabsf(bhi), 0x1p-21f, bhi);
                                    }
                                    // (all four finite: then no ray of the wave computes a NaN or an infinity here either; if not, this plane bounds nothing)
                                    const bool finite = fmaxf(fmaxf(fabsf(alo), fabsf(ahi)), fmaxf(fabsf(b0), fabsf(b1))) < __builtin_inff();
                                    const bool near = (is_max != 0u) == (cr.x < 0.0f);
                                    float bound = plane<NODE>(v, near ? alo : ahi, near ? blo : bhi);
                                    if (!finite) bound = near ? -__builtin_inff() : __builtin_inff();
                                    lds_cull[(dl & 7u) * 8u + (near ? 0u : 4u) + a] = bound;
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            uint32_t keep_children = 0xffu;
                            if (culling) {
                                const float4 *cb = reinterpret_cast<const float4 *>(lds_cull) + 2u * (lane & 7u);
                                const float4 lb = cb[0], ub = cb[1];
                                const float tmin_lb = fmaxf(fmaxf(fmaxf(lb.x, lb.y), lb.z), 0.0001f);
                                // (the largest t of the wave's rays as one more upper bound - a wave scan per step - measured slower,
                                // profiles/r05_ab_18_cull_final.log)
                                const float tmax_ub = fminf(fminf(ub.x, ub.y), ub.z);
                                keep_children = (uint32_t)__ballot(!(tmin_lb > tmax_ub)) & 0xffu; // (lanes 0..7 = children 0..7)
                                __builtin_amdgcn_wave_barrier();
                            }
                            if (kTune && kCull && (P.tune & 0x100u) && lane == 0u) // (diagnostics, tools/gpu_cullhist.py: children left by the packet test; 9 = no packet test)
                                atomicAdd(&P.ctr->hist_total[culling ? (uint32_t)__builtin_popcount(keep_children) : 9u], 1u);
                            if (act) {
                                const uint4 n1 = np[1];
                                cur.y &= ~(1u << child_bit);
                                stack_push(cur, (cur.y & 0xff000000u) != 0u);
                                // (the ray's view of the node's frame computed ahead of the barrier, under the bounds' trip through LDS: +0.8 %)
                                const uint32_t hitmask = node_intersect_kept<NODE>(r, t, node_frame<NODE>(r, n0, pow2), n1, lds_dec, lds_dec_neg, keep_children);
                                cur.x = n1.x;
                                tri.x = n1.y;
                                cur.y = (hitmask & 0xff000000u) | (n0.w >> 24);
                                tri.y = hitmask & 0x00ffffffu;
                            }
                            __builtin_amdgcn_wave_barrier();
                            lane_step = 0u;
                        } else if (kUniCool != 0u) {
                            uni_cool = kUniCool;
                        }
                    }
                }
                // (the per-lane step behind a scalar flag of its own.  The compiler must not know that the flag is the uniform
                // step's: as `act && !uni_done` the test after a uniform step was a mask of zeroes, an exec save and a branch
                // that is always taken, and as an if / else the two steps reach the assembly as two ifs under a mask of the
                // compiler's making, every word they define copied into the join.  Nor may it merge the scalar test into
                // the lanes' mask - four scalar instructions instead of a compare and a branch: the empty statement is a
                // side effect between the two tests.)
                asm("" : "+s"(lane_step));
                if (lane_step != 0u) { asm volatile("");
                if (act) {
                    if (group) { // (node_index, child_bit: from the head of the trip)
                        cur.y &= ~(1u << child_bit);
                        // (tried: when every lane wants the same node - 47 % of the wave-level steps on the bistro-class frame,
                        // 90 % on the kitchen-class one - one copy through the scalar cache instead of 64 through the vector
                        // path: no change in frame time; DESIGN.md section 4)
                        const uint4 *np = P.nodes + (size_t)node_index * 5;
                        const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3], n4 = np[4];
                        stack_push(cur, (cur.y & 0xff000000u) != 0u); // after the loads are on their way
                        TRX_STAMP(k_fetch);
                        if (COUNT) {
                            c_node++;
                            if (lane_rank(__ballot(1)) == 0) c_wnode++;
                            if (P.touch_nodes) P.touch_nodes[node_index] = 1;
                            if (kTune && (P.tune & 0x100u)) {
                                // diagnostics: distinct nodes among the lanes of this wave-level node step
                                unsigned long long todo = __ballot(1);
                                const uint32_t first = (uint32_t)__ffsll((long long)todo) - 1u;
                                uint32_t distinct = 0;
                                while (todo) {
                                    const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1u;
                                    const uint32_t v = (uint32_t)__shfl((int)node_index, (int)l);
                                    todo &= ~__ballot(node_index == v);
                                    distinct++;
                                }
                                if (lane == first) atomicAdd(&P.ctr->hist_total[min(distinct, 15u)], 1u);
                            }
                        }
                        const uint32_t hitmask = node_intersect<NODE>(r, t, n0, n1, n2, n3, n4, pow2);
                        cur.x = n1.x;
                        tri.x = n1.y;
                        cur.y = (hitmask & 0xff000000u) | (n0.w >> 24);
                        tri.y = hitmask & 0x00ffffffu;
                    } else {
                        tri = cur;
                        cur = make_uint2(0u, 0u);
                    }
                }
                } // (lane_step)
                // instance masks (trx_trace_*_masked*): an instance of the TLAS leaf group whose mask misses the call's ray
                // mask is dropped where the pick below would enter it, and the walk goes on as it would after entering an
                // EMPTY instance: with the TLAS node group `cur` if it holds children (the rest of the leaf group parked
                // under it), else with the next instance of the group.  So the TLAS visits everything else in the
                // unmasked order, and a group whose instances are all invisible enters nothing.  (P.inst_mask is a launch
                // argument, so the test is wave-uniform; the unmasked launches pass null and never run the loop.)
                if constexpr (TLAS) {
                    if (__builtin_expect(P.inst_mask != nullptr, 0) && act && tlas_sp == TRX_INVALID && tri.y != 0u) {
                        bool park = false;
                        while (tri.y != 0u) {
                            const uint32_t local = 31u - (uint32_t)__clz((int)tri.y);
                            if ((P.inst_mask[tri.x + local] & P.ray_mask) != 0u) break;
                            tri.y &= ~(1u << local);
                            if ((cur.y & 0xff000000u) != 0u) {
                                park = true;
                                break;
                            }
                        }
                        stack_push(tri, park && tri.y != 0u);
                        if (park) tri.y = 0u;
                    }
                }
                if (TLAS && act && tlas_sp == TRX_INVALID && tri.y != 0u) { // (after either kind of node step)
                    // a TLAS primitive is an instance (query_tlas.hlsl:410-446): enter its BLAS
                    const uint32_t local = 31u - (uint32_t)__clz((int)tri.y);
                    tri.y &= ~(1u << local);
                    const uint32_t gidx = tri.x + local;
                    stack_push(tri, tri.y != 0u);
                    stack_push(cur, (cur.y & 0xff000000u) != 0u);
                    tlas_sp = sp;
                    bvh_off = P.inst[gidx];
                    cur_inst = gidx;
                    if (P.inst_xform) {
                        // the ray in the instance's object space
                        const float4 *m = P.inst_xform + (size_t)gidx * 3;
                        const float4 r0 = m[0], r1 = m[1], r2 = m[2];
                        const float wox = wray[0 * kWave + lane], woy = wray[1 * kWave + lane], woz = wray[2 * kWave + lane];
                        const float wdx = wray[3 * kWave + lane], wdy = wray[4 * kWave + lane], wdz = wray[5 * kWave + lane];
                        TRX_RAY_TO_OBJECT(r0, r1, r2, wox, woy, woz, wdx, wdy, wdz, r.ox, r.oy, r.oz, odx, ody, odz)
                        finish_ray_dir<(NODE & 1) == 0>(r, odx, ody, odz);
                        TRX_PUBLISH_RAY();
                    }
                    // the walk of the BLAS starts at its node 0 (query_tlas.hlsl:443) - or, for a TLAS primitive that
                    // stands for a SUBTREE of its BLAS (re-braided scenes, trx_scene_set_instance_entry_nodes), at
                    // that subtree's node: the group {child_base = entry, one hit} makes the next node step fetch it
                    cur = make_uint2(P.inst_entry ? P.inst_entry[gidx] : 0u, 0x80000000u);
                    tri.y = 0u;
                }

                TRX_STAMP(k_test);
                triangle_phase(tri);
                TRX_STAMP(k_tri);
                if constexpr (kStamps) k_iters++;
                if constexpr (TLAS) {
                    // (the two-level kernels keep the per-lane form: with the scalar `done` mask of the single-level walk they
                    // park more scalars in vector lanes inside the loop than tests/test_kernel_resources.py allows)
                    if (act) {
                        // a lane whose node group is spent pops the next one, or is finished when its stack is empty
                        const bool spent = (cur.y & 0xff000000u) == 0u;
                        bool done = spent && sp == 0u;
                        if (spent && sp != 0u) {
                            if (sp == tlas_sp) { // back to the TLAS (query_tlas.hlsl:480-486)
                                tlas_sp = TRX_INVALID;
                                bvh_off = P.tlas_start;
                                cur_inst = TRX_INVALID;
                                if (P.inst_xform) { // "Reset Ray to untransformed version" (query_tlas.hlsl:484)
                                    r.ox = wray[0 * kWave + lane]; r.oy = wray[1 * kWave + lane]; r.oz = wray[2 * kWave + lane];
                                    finish_ray_dir<(NODE & 1) == 0>(r, wray[3 * kWave + lane], wray[4 * kWave + lane], wray[5 * kWave + lane]);
                                    TRX_PUBLISH_RAY();
                                }
                            }
                            cur = stack_pop();
                            if (__builtin_expect(overflow != 0u, 0)) done = true; // past the last stack entry: the sentinel is not a group
                        }
                        // step cap (every wave reaches an exit whatever the tree): a ray's steps are bounded by the wave's
                        // trips since it started; looked at once per 1024 trips, so the common trip pays nothing for it
                        if (__builtin_expect((trip & 1023u) == 0u, 0)) {
                            if (trip - steps > kMaxSteps) {
                                overflow = 1u;
                                done = true;
                            }
                        }
                        // any-hit query (intersects_bl_bvh, query.hlsl:440-445): the first accepted triangle settles it.
                        // Until a hit is accepted the walk is the closest-hit walk, so hit / no hit is the same answer.
                        if (MODE == kModeRays && P.any_hit != 0u && prim != TRX_INVALID) done = true;
                        if (done) finish_lane();
                    }
                } else {
                    // a lane whose node group is spent pops the next one, or is finished when its stack is empty - or
                    // when it has gone past the last stack entry: the sentinel it pops is not a group
                    // (layout: `done` is a scalar mask and the WAVE asks once whether any lane is done, so a trip in which
                    // none finishes falls through - no branch round the overflow check after a pop, no exec save round the
                    // end of a ray.  The mask is made of ballots of ONE comparison each, taken by every lane and cut to
                    // the lanes with a ray by the scalar unit: the ballot of a combined condition goes through a 0 / 1
                    // register and a second comparison, and a mask assigned under `if (act)` is a per-lane value to the
                    // compiler - a register pair and a 64-bit vector comparison.)
                    const bool spent = (cur.y & 0xff000000u) == 0u;
                    unsigned long long done = ballot64(spent) & (ballot64(sp == 0u) | ballot64(overflow != 0u)) & act_mask;
                    if (act && spent && sp != 0u) cur = stack_pop();
                    // any-hit query, as above
                    if (MODE == kModeRays && P.any_hit != 0u) done |= ballot64(prim != TRX_INVALID) & act_mask;
                    // step cap, as above
                    if (__builtin_expect((trip & 1023u) == 0u, 0)) {
                        const bool capped = trip - steps > kMaxSteps;
                        if (act && capped) overflow = 1u;
                        done |= ballot64(capped) & act_mask;
                    }
                    if (__builtin_expect(done != 0ull, 0)) {
                        if (__builtin_amdgcn_inverse_ballot_w64(done)) finish_lane(); // (the scalar mask as the lanes' condition: one exec save, no lane-bit registers)
                    }
                }
                const uint32_t alive = (uint32_t)__popcll(ballot64(has_ray));
                TRX_STAMP(k_pop);
                if (kMerge && merge_open && exhausted) {
                    merge_step(alive);
                    if (__ballot(has_ray) == 0ull) break;
                    continue;
                }
                if (alive <= (TLAS ? (exhausted ? 0u : keep) : leave_at)) break; // (no lane left, or - queues not dry - few enough to go and refill)
                // fused frame, queues dry: waiting lanes are turned into AO rays once enough of them have gathered
                if (kFused && exhausted && (uint32_t)__popcll(__ballot(pend)) >= P.pend_min) break;
                if (kThin && thin_now(alive)) {
                    go_thin = true;
                    break;
                }
            }

