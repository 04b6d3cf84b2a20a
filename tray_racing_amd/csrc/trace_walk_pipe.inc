// trace_walk_pipe.inc - part of k_trace (kernels.hip), included as text inside the kernel: the pipelined walk (incoherent single-level passes): next node's fetch under the triangle phase
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
            // Pipelined walk (BLAS only).  Per trip: (1) lanes whose group names a next node issue its fetch and push
            // the group's remainder; (2) the triangle phase of the node tested in the PREVIOUS trip runs under those
            // loads; (3) rays with nothing left to fetch are finished (their last triangles are in); (4) the node test
            // of the fetched node, with the t the triangles left, and the pop of a spent group.  Stack traffic, node
            // order, triangle order and the t every test sees are those of the plain walk.
            for (;;) {
                const bool act = has_ray;
                const int pow2 = (NODE & 1) ? 0 : pow2_exact(P, r, act); // (literal-division variants only)
                trip++;
                if (!TLAS && MODE != kModePrimary && (trip & 7u) == 0u) old_ray_priority(); // (measured without effect in the two-level kernels)
                // The fetched node record lives from (1) to (4) of ONE trip and is deliberately left uninitialised here:
                // carried across trips (a variable of the kernel, as it was) the five loads merge with the previous
                // trip's values, the register allocator is free to land them in scratch registers and copy them home at
                // once - and that copy waits for the loads thirteen instructions after they were issued instead of a
                // triangle phase later.  Round 4 shipped that for a while (AO passes +5-8 %): tests/test_kernel_resources.py
                // now measures the distance from the fetch to the first wait in the compiled walk.
                uint4 fn0, fn1, fn2, fn3, fn4;
                // (1)
                if (act && !fetched && (cur.y & 0xff000000u)) {
                    const uint32_t hits_imask = cur.y;
                    const uint32_t child_bit = 31u - (uint32_t)__builtin_clz(hits_imask);
                    const uint32_t child_base = cur.x;
                    cur.y &= ~(1u << child_bit);
                    const uint32_t slot = (child_bit - 24u) ^ (r.oct_inv4 & 0xffu);
                    const uint32_t rel = (uint32_t)__popc(hits_imask & ~(0xffffffffu << slot));
                    const uint32_t node_index = child_base + rel;
                    const uint4 *np = P.nodes + (size_t)node_index * 5;
                    fn0 = np[0]; fn1 = np[1]; fn2 = np[2]; fn3 = np[3];
                    {   // (the last 16 bytes as two 8-byte loads: pairs of registers are easier to keep than a fifth quadruple)
                        const uint2 *h = reinterpret_cast<const uint2 *>(np + 4);
                        const uint2 a = h[0], b = h[1];
                        fn4 = make_uint4(a.x, a.y, b.x, b.y);
                    }
                    stack_push(cur, (cur.y & 0xff000000u) != 0u); // after the loads are on their way
                    fetched = true;
                    if (COUNT) {
                        c_node++;
                        if (lane_rank(__ballot(1)) == 0) c_wnode++;
                        if (P.touch_nodes) P.touch_nodes[node_index] = 1;
                    }
                }
                TRX_STAMP(k_fetch);
                // (2)
                triangle_phase(ptri);
                ptri = make_uint2(0u, 0u);
                TRX_STAMP(k_tri);
                if constexpr (kStamps) k_iters++;
                // (3)
                if (act) {
                    bool done = !fetched; // no node left to visit, and the last node's triangles are in
                    if (MODE == kModeRays && P.any_hit != 0u && prim != TRX_INVALID) done = true;
                    if (__builtin_expect((trip & 1023u) == 0u, 0)) { // step cap: every wave reaches an exit
                        if (trip - steps > kMaxSteps) {
                            overflow = 1u;
                            done = true;
                        }
                    }
                    if (done) {
                        fetched = false; // a fetch still in flight (any-hit, step cap) is simply not looked at
                        finish_lane();
                    }
                }
                const uint32_t alive = (uint32_t)__popcll(__ballot(has_ray));
                const bool leave = alive == 0u || (!exhausted && alive <= keep);
                TRX_STAMP(k_pop);
                // (4)
                if (fetched) {
                    const uint32_t hitmask = node_intersect<NODE>(r, t, fn0, fn1, fn2, fn3, fn4, pow2);
                    cur.x = fn1.x;
                    ptri.x = fn1.y;
                    cur.y = (hitmask & 0xff000000u) | (fn0.w >> 24);
                    ptri.y = hitmask & 0x00ffffffu;
                    fetched = false;
                    if ((cur.y & 0xff000000u) == 0u && sp != 0u) {
                        cur = stack_pop();
                        if (__builtin_expect(overflow != 0u, 0)) cur = make_uint2(0u, 0u); // past the last entry: finish
                    }
                }
                TRX_STAMP(k_test);
                if (kMerge && merge_open && exhausted) {
                    merge_step(alive);
                    if (__ballot(has_ray) == 0ull) break;
                    continue;
                }
                if (leave) break;
                if (kFused && exhausted && (uint32_t)__popcll(__ballot(pend)) >= P.pend_min) break;
                if (kThin && thin_now(alive)) {
                    go_thin = true;
                    break;
                }
            }
