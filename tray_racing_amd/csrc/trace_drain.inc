// trace_drain.inc - part of k_trace (kernels.hip), included as text inside the kernel: the drain - hand-over between the two waves of a workgroup, priority by ray age
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
        // The second wave of a draining workgroup offers its rays (see "The drain" above); true = taken over, this wave is empty.
        auto merge_offer = [&](uint32_t alive) -> bool {
            const uint32_t avail = *reinterpret_cast<volatile uint32_t *>(&merge_ctl[1]);
            if (avail < alive || __ballot(has_ray && sp > (uint32_t)kLdsStack) != 0ull) return false; // (stacks past the LDS part stay)
            const uint32_t j = lane_rank(__ballot(has_ray));
            if (has_ray) {
                uint32_t *m = merge_box + j * kMergeWords;
                m[0] = __float_as_uint(r.ox); m[1] = __float_as_uint(r.oy); m[2] = __float_as_uint(r.oz);
                m[3] = __float_as_uint(r.dx); m[4] = __float_as_uint(r.dy); m[5] = __float_as_uint(r.dz);
                m[6] = __float_as_uint(r.ix); m[7] = __float_as_uint(r.iy); m[8] = __float_as_uint(r.iz);
                m[9] = __float_as_uint(r.tmin); m[10] = r.oct_inv4;
                m[11] = __float_as_uint(t); m[12] = prim; m[13] = out_index; m[14] = trip - steps;
                m[15] = cur.x; m[16] = cur.y; m[17] = sp; m[18] = ptri.x; m[19] = ptri.y; m[20] = lane;
                if (TLAS) {
                    m[21] = bvh_off; m[22] = tlas_sp; m[23] = cur_inst; m[24] = hit_inst;
                    for (int c = 0; c < 6; c++) m[25 + c] = __float_as_uint(wray[c * kWave + lane]); // (a ray's world-space copy travels with it)
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            uint32_t old = 0u;
            if (lane == 0u) old = atomicCAS(&merge_ctl[0], 0u, alive);
            old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
            merge_open = false; // one offer per wave
            if (old != 0u) { // the first wave has left: finish them here (the parking area covered this wave's ray copies)
                if (has_ray) {
                    TRX_PUBLISH_RAY();
                }
                return false;
            }
            has_ray = false;
            return true;
        };
        // The first wave takes what the second offered, if anything (n = control word 0).
        auto merge_take = [&](uint32_t n) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const uint32_t j = lane_rank(__ballot(!has_ray));
            if (!has_ray && j < n) {
                const uint32_t *m = merge_box + j * kMergeWords;
                r.ox = __uint_as_float(m[0]); r.oy = __uint_as_float(m[1]); r.oz = __uint_as_float(m[2]);
                r.dx = __uint_as_float(m[3]); r.dy = __uint_as_float(m[4]); r.dz = __uint_as_float(m[5]);
                r.ix = __uint_as_float(m[6]); r.iy = __uint_as_float(m[7]); r.iz = __uint_as_float(m[8]);
                r.tmin = __uint_as_float(m[9]); r.oct_inv4 = m[10];
                t = __uint_as_float(m[11]); prim = m[12]; out_index = m[13]; steps = trip - m[14];
                cur = make_uint2(m[15], m[16]); sp = m[17]; ptri = make_uint2(m[18], m[19]);
                if (TLAS) {
                    bvh_off = m[21]; tlas_sp = m[22]; cur_inst = m[23]; hit_inst = m[24];
                    for (int c = 0; c < 6; c++) wray[c * kWave + lane] = __uint_as_float(m[25 + c]);
                }
                const uint32_t from = m[20];
                for (uint32_t k = 0; k < sp; k++) lds_st(&lds_stack[k * kWave + lane], merge_stack1[k * kWave + from]);
                TRX_PUBLISH_RAY();
                fetched = false;
                overflow = 0u;
                has_ray = true;
            }
            merge_open = false;
        };
        // End of a trip of a dry wave: the second wave offers once its rays fit the first one's idle lanes; the first
        // publishes its idle lanes and looks for an offer.
        auto merge_step = [&](uint32_t alive) {
            if (wave_in_block == 1u) {
                // (a wave that is down to a handful of rays finishes them itself, eight lanes to a ray - thin_walk - rather
                // than hand them to a wave that steps them one lane each)
                if (kThin && alive <= P.thin_max) merge_open = false;
                else if (alive != 0u && alive <= kMergeMax) (void)merge_offer(alive);
            } else {
                if (lane == 0u) *reinterpret_cast<volatile uint32_t *>(&merge_ctl[1]) = (uint32_t)kWave - alive;
                const uint32_t n = *reinterpret_cast<volatile uint32_t *>(&merge_ctl[0]);
                if (n != 0u) {
                    merge_take(n);
                } else if (kThin && alive <= P.thin_max) {
                    // ... and the first wave, down to a handful, closes the door - unless an offer has just landed
                    uint32_t old = 0u;
                    if (lane == 0u) old = atomicCAS(&merge_ctl[0], 0u, kMergeClosed);
                    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
                    if (old == 0u) merge_open = false;
                    else merge_take(old);
                }
            }
        };

        // Incoherent passes end when their longest rays do (a third of the hairball-class AO pass's wave time is waves
        // waiting for them, and dealing the tiles longest ray first does not move that tail: profiles/r03_ao_order.log, tools/gpu_timeline_ao.py), so
        // a wave that holds an old ray wins the issue arbitration of its SIMD: priority 2 once its oldest ray has run
        // kOldRay trips, 3 from twice that, looked at every eighth trip.  Worth 1-2 % of an AO pass (four alternating
        // repetitions on four scenes, all four means lower; the run-to-run spread of an AO pass is +-2 %).  The threshold is
        // not a lever: 32 / 64 / 128 / 256 trips measure within 0.3 % of each other on every pass (profiles/r06_ab_old_ray.log).
#ifndef TRX_OLD_RAY
#define TRX_OLD_RAY 32
#endif
        constexpr uint32_t kOldRay = (TRX_OLD_RAY);
        auto old_ray_priority = [&]() {
            const uint32_t age = has_ray ? trip - steps : 0u;
            if (__ballot(age >= 2u * kOldRay) != 0ull) __builtin_amdgcn_s_setprio(3);
            else if (__ballot(age >= kOldRay) != 0ull) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(0);
        };

