// trace_stack.inc - part of k_trace (kernels.hip), included as text inside the kernel: the per-lane stack (LDS, then HBM) and the end of a ray
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
    // (defined out here, ahead of the loop, because the thin walk also runs after it: see the end of the loop)
    // Stack push / pop.  Fast path: every lane's top is inside the LDS part, so the write needs no
    // predication at all (an entry above a lane's top is free to clobber) and the whole push is one
    // ds_write_b64 plus a conditional increment; lanes past the LDS part (rare: depth > kLdsStack) take the
    // general path behind a wave-uniform branch.
    auto stack_push = [&](uint2 e, bool cond) {
        if (__builtin_expect(__ballot(sp >= (uint32_t)kLdsStack) != 0ull, 0)) {
            if (cond) {
                if (sp < (uint32_t)kLdsStack) lds_st(&lds_stack[sp * kWave + lane], e);
                else if (sp < (uint32_t)(kLdsStack + kSpillStack)) spill[(sp - kLdsStack) * kWave + lane] = e;
                else overflow = 1u;
            }
        } else {
            lds_st(&lds_stack[sp * kWave + lane], e);
        }
        sp += cond ? 1u : 0u;
        if (COUNT) c_maxsp = max(c_maxsp, sp);
    };
    // (the pop has no `else`: a wave-uniform if / else whose arms hold per-lane branches reaches the assembly as two ifs in a
    // row under a flag of the compiler's making, the common arm - the LDS read - behind a branch that is always taken.  The
    // LDS read is unconditional - a lane past the LDS part reads its own last LDS entry and drops it - and the rare path
    // is an if of its own.  The same form for the push - its common store behind an opaque flag - measured inside one
    // spread and was not kept, profiles/walk_scalar_cost.log.)
    auto stack_pop = [&]() -> uint2 { // callers guarantee sp != 0
        sp--;
        uint2 e = lds_ld(&lds_stack[min(sp, (uint32_t)(kLdsStack - 1)) * kWave + lane]);
        if (__builtin_expect(__ballot(sp >= (uint32_t)kLdsStack) != 0ull, 0)) {
            if (sp >= (uint32_t)kLdsStack) {
                e = make_uint2(0u, 0u); // (past the last entry: the sentinel)
                if (sp < (uint32_t)(kLdsStack + kSpillStack)) e = spill[(sp - kLdsStack) * kWave + lane];
            }
        }
        return e;
    };

    // Finished ray: the hit record (or the any-hit flag) leaves the lane.
    auto finish_lane = [&]() {
        if constexpr (MODE == kModeService) {
            // the answer goes straight into the slot's answer words in host memory - ONE 16-byte store {t, prim, overflow,
            // seq} (an overflowed stack / the step cap travels with the answer: it is this caller's error, not a sticky flag
            // of the launch slot) - and the sequence number into the mailbox, which tells the workgroup's porter that the slot
            // may take its next request
            // (word 2: bit 0 = overflow; for the service's statistics bits 1..15 = 100 MHz ticks from the ray's admission to
            // here, bits 16..31 = its trips of the walk)
            const uint32_t ticks = (uint32_t)min(wall_clock64() - svc_t0, 32767ull), trips_w = min(trip - steps, 65535u);
            const u32x4 a = {prim != TRX_INVALID ? __float_as_uint(t) : 0x7f800000u, prim, (overflow & 1u) | (ticks << 1) | (trips_w << 16), svc_seq};
            uint32_t *ans = P.svc_ring + (size_t)(blockIdx.x * kSvcRays + (lane >> 3)) * kSvcSlotWords + 16;
            if constexpr (TLAS) { // (two-level scenes: the TLAS primitive the hit was found in, a granule of its own beside the answer)
                const u32x4 b = {prim != TRX_INVALID ? hit_inst : TRX_INVALID, 0u, 0u, svc_seq};
                asm volatile("global_store_dwordx4 %0, %1, off offset:16 sc0 sc1" : : "v"(ans), "v"(b) : "memory");
            }
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(ans), "v"(a) : "memory");
            svc_box[128u + 4u * (lane >> 3) + 3u] = svc_seq;
            has_ray = false;
            return;
        } else
        if (MODE == kModeRays && P.any_hit != 0u) {
            reinterpret_cast<uint8_t *>(P.out)[out_index] = prim != TRX_INVALID ? 1u : 0u;
        } else {
            trx_hit h;
            h.t = prim != TRX_INVALID ? t : __builtin_inff();
            h.prim = prim;
            const uint32_t hi = prim != TRX_INVALID ? hit_inst : TRX_INVALID;
            if (kFused && is_ao) {
                P.out_ao[out_index] = h;
                if (TLAS && P.out_ao_inst) P.out_ao_inst[out_index] = hi;
            } else {
                P.out[out_index] = h;
                if (TLAS && P.out_inst) P.out_inst[out_index] = hi;
                if (kFused) {
                    // the reference's pixel program goes on with the AO ray when the primary ray hit
                    // (rt_gpu_software.hlsl:105); a miss ends the pixel: its AO record is a miss as well
                    if (prim != TRX_INVALID) {
                        pend = true;
                    } else {
                        P.out_ao[out_index] = h;
                        if (TLAS && P.out_ao_inst) P.out_ao_inst[out_index] = TRX_INVALID;
                    }
                }
            }
        }
        if (COUNT) {
            c_rays++;
            c_hits += prim != TRX_INVALID;
        }
        // this ray's share of n_node / n_tri, saturated like the per-ray counters of the CPU restatement
        // (if constexpr: in the timed kernels the lambda then names - and captures - nothing more than it did)
        if constexpr (COUNT)
            if (ray_cost) ray_cost[out_index] = trx_ray_cost{(uint16_t)min(c_node - r_node, 65535u), (uint16_t)min(c_tri - r_tri, 65535u)};
        c_over += overflow;
        has_ray = false;
    };

