// build_levels.h - the level lists of a BVH2 on the device, top-down (frontier expansion): the kernel and the host loop
// that collapse_gpu.cpp and reinsert_gpu.cpp both run before they work level by level.  HIP only.
#pragma once
#include "build_device.h"

namespace trx {

// The children of the inner nodes of one level are the next level.
// (capacity = entries `out` can take: links that do not describe a tree - the very case the host loop below reports - must
// not turn into stores past the list; an append that does not fit is dropped, the counter still says how many were wanted)
static __global__ __launch_bounds__(kBlock) void k_expand_level(const Node2 *nodes, const uint32_t *in, uint32_t n_in, uint32_t *out,
                                                                 uint32_t *counter, uint32_t capacity) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t left = 0, right = 0, prim, count = 0;
    if (t < n_in) load_links(nodes, in[t], left, right, prim, count);
    const bool inner = count > 1;
    const uint32_t at = wave_append(counter, inner ? 2u : 0u);
    if (inner && at + 2u <= capacity) {
        out[at] = left;
        out[at + 1] = right;
    }
}

// Fills d_list (n entries) with the n nodes below node 0, level after level: level L = d_list[level[L] .. level[L + 1]).
// d_counter: one word of device memory.  Fails with `who` in the message where the links are not a tree of n nodes.
inline bool expand_levels(const char *who, const Node2 *d_nodes, uint32_t n, uint32_t *d_list, uint32_t *d_counter,
                          std::vector<uint32_t> &level, std::string &err) {
    level.assign({0u, 1u});
    const uint32_t zero = 0;
    TRX_BUILD_TRY(hipMemcpy(d_list, &zero, 4, hipMemcpyHostToDevice));
    for (;;) {
        const uint32_t begin = level[level.size() - 2], end = level.back();
        if (end == begin) {
            level.pop_back();
            break;
        }
        if (end >= n) break; // every node is listed: the last level holds leaves only
        TRX_BUILD_TRY(hipMemsetAsync(d_counter, 0, 4, nullptr));
        hipLaunchKernelGGL(k_expand_level, grid_for(end - begin), dim3(kBlock), 0, nullptr, d_nodes, d_list + begin, end - begin, d_list + end,
                           d_counter, (uint32_t)(n - end));
        TRX_BUILD_TRY(hipGetLastError());
        uint32_t made = 0;
        TRX_BUILD_TRY(hipMemcpy(&made, d_counter, 4, hipMemcpyDeviceToHost));
        if ((size_t)end + made > n) {
            err = std::string(who) + ": the links do not describe a tree of n_nodes nodes";
            return false;
        }
        level.push_back(end + made);
    }
    if (level.back() != n) {
        err = std::string(who) + ": " + std::to_string(n - level.back()) + " nodes are not reachable from node 0";
        return false;
    }
    return true;
}

} // namespace trx
