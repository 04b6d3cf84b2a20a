// trace_service.inc - part of k_trace (kernels.hip), included as text inside the kernel: the ray service (MODE == kModeService)
// (One function for the compiler - the pieces share fifty live variables - several files for the reader.)
        // kernels.h (kSvcRays) has the protocol.  Workgroup = two waves: wave 0 walks (thin_walk with its step (0)), wave 1 is
        // the porter below.  Both come back here and run the epilogue (the exit ticket counts every wave of the grid).
        if (wave_in_block == 1u) {
            // The porter looks into host memory with SCALAR loads - everything below is wave-uniform.  Vector loads did the
            // job until late in round 6 and cost the walker half its speed: a CU's vector-memory path returns a wave's cache
            // hits behind other waves' requests in flight (tools/ubench/tcp_order.hip: a dependent hit 180 cycles alone, 452
            // beside one HBM miss of another wave of the CU, 854 beside a read of pinned host memory - and 181 beside the same
            // read through the scalar cache), so every node and triangle request of the walker queued behind the porter's
            // reads of the ring, 1-2 us each, back to back: 1 830 of a trip's 3 400 cycles were the wait for a node record
            // that sat in the L2 (tuning build -DTRX_SVC_PHASES).
            static_assert(kSvcRays == 4 && kSvcSlotWords == 32, "the offsets below: four 128-byte slots, three 16-byte granules each");
            const uint32_t *const ring_base = P.svc_ring + (size_t)(blockIdx.x * kSvcRays) * kSvcSlotWords;
            // what a slot's last answer was: a request with another number is one nobody has answered yet (a service that is
            // started again finds the numbers of its predecessor in the ring)
            uint32_t adm[kSvcRays], wr[kSvcRays];
            {
                const uint32_t mine = lane < kSvcRays ? sys_load128(ring_base + lane * kSvcSlotWords + 16).w : 0u;
                for (uint32_t k = 0; k < kSvcRays; k++) adm[k] = wr[k] = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)k);
                if (lane < kSvcRays) {
                    svc_box[16u * lane + 12u] = mine;
                    svc_box[128u + 4u * lane + 3u] = mine;
                }
            }
            if (lane == 0u) svc_box[192] = 0u;
            __syncthreads();
            unsigned long long beat_t = wall_clock64();
            uint32_t beat = 0u;
            bool first_look = true;
            uint32_t quiet = 0u; // looks since the workgroup last had a request in hand
            uint32_t look = 0u;
            for (;;) {
                // ---- requests: the four slots' request lines and the control words, five reads in flight together.  A request
                // is whole when its three granules carry the same number, and new when the slot's last answer carries another.
                // (ONE 64-byte read per slot - its request line - and one for the control words: five reads per look and
                // porter.  Twelve 16-byte reads measured slower by 2.6 us a call with sixteen porters looking at once - a lone
                // wave's reads of host memory overlap perfectly, tools/ubench/host_poll.hip, the link's read queue does not
                // take 200 of them at a time.)
                u32x16 ra, rb, rc, rd;
                unsigned long long cw;
                asm volatile("s_load_dwordx16 %0, %5, 0x0 glc\n\t"
                             "s_load_dwordx16 %1, %5, 0x80 glc\n\t"
                             "s_load_dwordx16 %2, %5, 0x100 glc\n\t"
                             "s_load_dwordx16 %3, %5, 0x180 glc\n\t"
                             "s_load_dwordx2 %4, %6, 0x0 glc\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&s"(ra), "=&s"(rb), "=&s"(rc), "=&s"(rd), "=&s"(cw)
                             : "s"(ring_base), "s"(P.svc_ctl)
                             : "memory");
                const bool ctl_look = (look++ & 63u) == 0u;
                bool busy = false;
                auto take = [&](uint32_t k, const u32x16 &q) { // (q: words 0..3, 4..7, 8..11 = the three granules)
                    if (adm[k] == wr[k] && q.s3 == q.s7 && q.s7 == q.sb && q.s3 != adm[k]) {
                        // words [16 k .. 16 k + 8] = {ox oy oz dx dy dz tmin tmax}, one word per lane
                        const uint32_t v = lane == 0u ? q.s0 : lane == 1u ? q.s1 : lane == 2u ? q.s2 : lane == 3u ? q.s4 : lane == 4u ? q.s5 : lane == 5u ? q.s6 : lane == 6u ? q.s8 : q.s9;
                        if (lane < 8u) svc_box[16u * k + lane] = v;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0u) svc_box[16u * k + 12u] = q.s3;
                        adm[k] = q.s3;
                    }
                    busy |= adm[k] != wr[k];
                };
                take(0u, ra);
                take(1u, rb);
                take(2u, rc);
                take(3u, rd);
                // ---- answers: the walker stores its record into the slot's answer words itself (one 16-byte store per ray;
                // relayed through this wave it waited up to a whole look, 2-4 us); its number in the mailbox says that the
                // slot may take the next request
                for (uint32_t k = 0; k < kSvcRays; k++) wr[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)svc_box[128u + 4u * k + 3u]);
                // (a workgroup nobody has talked to for a while looks less often: sixteen porters reading pinned host memory
                // flat out are traffic on the link that the callers' own requests and answers cross)
                if (busy) quiet = 0u;
                else if (quiet < 256u) quiet++;
                else __builtin_amdgcn_s_sleep(64);
                // ---- control: leave when told to, or when the host's heartbeat has stood still for two seconds
                if (ctl_look) {
                    const uint32_t leave = (uint32_t)cw, hb = (uint32_t)(cw >> 32);
                    const unsigned long long now = wall_clock64();
                    if (first_look || hb != beat) {
                        beat = hb;
                        beat_t = now;
                        first_look = false;
                    }
                    if (leave != 0u || now - beat_t > kSvcDeadTicks) {
                        if (lane == 0u) svc_box[192] = 1u;
                        break;
                    }
                }
            }
        } else {
            __syncthreads(); // (the porter has set the mailboxes' numbers)
            svc_seq = (lane >> 3) < kSvcRays ? svc_box[16u * (lane >> 3) + 12u] : 0u;
            thin_walk();
        }
