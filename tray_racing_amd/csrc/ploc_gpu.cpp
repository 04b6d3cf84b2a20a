// ploc_gpu.cpp — the BVH2 stage of the ploc_cwbvh build on the GPU (gfx950): Morton codes, radix sort and the PLOC
// merge rounds (Meister & Bittner 2018) as kernels.  The code grid, the codes, the neighbour choice with its tie rules and
// the box unions are build_rules.h's, the very functions PlocBuilder::run in builder.cpp calls, so the tree it returns is
// THE tree the CPU stage returns, node for node (tests/test_gpu_builder.py compares them).
//
// What it stands in for: the BVH2 build inside obvhs build_cwbvh_from_tris (src/cwbvh.rs:97), parameters
// src/main.rs:571-585 (ploc_search_distance, search_depth_threshold, sort_precision).
#include "ploc_gpu.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "build_device.h"

namespace trx {
namespace {

// bits == 21: one 63-bit key in key_lo.  bits == 42: the 126-bit key as (key_hi << 64) | key_lo, where the spread of
// the low 21 bits of each axis fills bits 0..62 and the spread of the high 21 bits starts at bit 63 (morton_key42)
__global__ void k_morton(const float *cen, uint32_t n, MortonFrame mp, int bits, uint64_t *key_lo, uint64_t *key_hi,
                         uint32_t *index) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t q[3];
    for (int k = 0; k < 3; k++) q[k] = morton_quant(cen[3 * (size_t)i + k], mp.lo[k], mp.scale[k]);
    index[i] = i;
    if (bits == 21) {
        key_lo[i] = morton_key21(q);
    } else {
        uint64_t l, h;
        morton_key42(q, l, h);
        key_lo[i] = l | (h << 63);
        key_hi[i] = h >> 1;
    }
}

__global__ void k_gather_keys(const uint64_t *src, const uint32_t *index, uint32_t n, uint64_t *dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[index[i]];
}

__global__ void k_leaves(const Aabb *boxes, const uint32_t *order, uint32_t n, Node2 *nodes, uint32_t *cluster, Aabb *cbox) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Node2 leaf;
    leaf.box = boxes[order[i]];
    leaf.left = leaf.right = 0;
    leaf.prim = order[i];
    leaf.count = 1;
    nodes[i] = leaf;
    cluster[i] = i;
    cbox[i] = leaf.box;
}

__global__ void k_nearest(const Aabb *cbox, uint32_t m, uint32_t r, uint32_t *nn) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    nn[i] = ploc_nearest(i, m, r, [&](uint32_t j) { return cbox[j]; });
}

// per cluster: low word = it survives into the next round (kept, or the first of a merging pair), high word = it
// starts a merge (a new node is created); an exclusive scan of the packed words gives both positions at once
__global__ void k_flags(const uint32_t *nn, uint32_t m, uint64_t *flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t j = nn[i];
    const bool mutual = nn[j] == i;
    const uint64_t keep = (!mutual || i < j) ? 1ull : 0ull;
    const uint64_t merge = (mutual && i < j) ? 1ull : 0ull;
    flags[i] = keep | (merge << 32);
}

__global__ void k_apply(const uint32_t *nn, const uint64_t *flags, const uint64_t *scan, uint32_t m, uint32_t next_node,
                        const uint32_t *cluster, const Aabb *cbox, Node2 *nodes, uint32_t *cluster_out, Aabb *cbox_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t f = flags[i];
    if (!(f & 1ull)) return; // the second of a merging pair disappears
    const uint32_t pos = (uint32_t)(scan[i] & 0xffffffffull);
    if (f >> 32) {
        const uint32_t j = nn[i];
        Node2 p;
        p.left = cluster[i];
        p.right = cluster[j];
        p.box = cbox[i];
        grow(p.box, cbox[j]);
        p.prim = 0;
        p.count = 0; // filled on the host (children precede their parent in creation order)
        const uint32_t id = next_node + (uint32_t)(scan[i] >> 32);
        nodes[id] = p;
        cluster_out[pos] = id;
        cbox_out[pos] = p.box;
    } else {
        cluster_out[pos] = cluster[i];
        cbox_out[pos] = cbox[i];
    }
}

} // namespace

bool ploc_bvh2_device(int device, const Aabb *boxes, const float *centroids, uint32_t n, uint32_t radius,
                      uint32_t depth_threshold, uint32_t sort_bits, void *nodes_out, uint32_t *root_out, double *seconds,
                      std::string &err) {
    if (n < 2) {
        err = "ploc_bvh2_device needs at least two primitives";
        return false;
    }
    DeviceScope scope;
    if (!scope.enter(device, err)) return false;
    Event ev0, ev1;
    TRX_BUILD_TRY(ev0.create());
    TRX_BUILD_TRY(ev1.create());
    const int bits = sort_bits == 128 ? 42 : 21;
    const MortonFrame mp = morton_frame(centroids, n, bits);

    const size_t total = 2 * (size_t)n - 1;
    DevBuf<Aabb> d_boxes, d_cbox_a, d_cbox_b;
    DevBuf<float> d_cen;
    DevBuf<Node2> d_nodes;
    DevBuf<uint64_t> d_key_a, d_key_b, d_key_hi, d_flags, d_scan;
    DevBuf<uint32_t> d_idx_a, d_idx_b, d_cluster_a, d_cluster_b, d_nn;
    DevBuf<unsigned char> d_tmp;
    TRX_BUILD_TRY(d_boxes.alloc(n));
    TRX_BUILD_TRY(d_cen.alloc(3 * (size_t)n));
    TRX_BUILD_TRY(d_nodes.alloc(total));
    for (DevBuf<uint64_t> *b : {&d_key_a, &d_key_b, &d_key_hi, &d_flags, &d_scan}) TRX_BUILD_TRY(b->alloc(n));
    for (DevBuf<uint32_t> *b : {&d_idx_a, &d_idx_b, &d_cluster_a, &d_cluster_b, &d_nn}) TRX_BUILD_TRY(b->alloc(n));
    TRX_BUILD_TRY(d_cbox_a.alloc(n));
    TRX_BUILD_TRY(d_cbox_b.alloc(n));
    TRX_BUILD_TRY(hipMemcpy(d_boxes.get(), boxes, (size_t)n * sizeof(Aabb), hipMemcpyHostToDevice));
    TRX_BUILD_TRY(hipMemcpy(d_cen.get(), centroids, (size_t)n * 12, hipMemcpyHostToDevice));

    size_t tmp_sort = 0, tmp_scan = 0;
    TRX_BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, d_key_a.get(), d_key_b.get(), d_idx_a.get(),
                                              d_idx_b.get(), (int)n, 0, 64, nullptr));
    TRX_BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, d_flags.get(), d_scan.get(), (int)n, nullptr));
    const size_t tmp_bytes = std::max<size_t>(std::max(tmp_sort, tmp_scan), 16); // (never 0: a null buffer asks hipcub for the size)
    TRX_BUILD_TRY(d_tmp.alloc(tmp_bytes));

    TRX_BUILD_TRY(hipEventRecord(ev0.get(), nullptr));
    // Morton order (stable LSD radix sort; 128-bit codes as two stable passes, low word first)
    hipLaunchKernelGGL(k_morton, grid_for(n), dim3(kBlock), 0, nullptr, d_cen.get(), n, mp, bits, d_key_a.get(),
                       d_key_hi.get(), d_idx_a.get());
    size_t tb = tmp_bytes;
    TRX_BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.get(), tb, d_key_a.get(), d_key_b.get(), d_idx_a.get(),
                                              d_idx_b.get(), (int)n, 0, 64, nullptr));
    uint32_t *order = d_idx_b.get();
    if (bits == 42) {
        hipLaunchKernelGGL(k_gather_keys, grid_for(n), dim3(kBlock), 0, nullptr, d_key_hi.get(), d_idx_b.get(), n,
                           d_key_a.get());
        tb = tmp_bytes;
        TRX_BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.get(), tb, d_key_a.get(), d_key_b.get(), d_idx_b.get(),
                                                  d_idx_a.get(), (int)n, 0, 64, nullptr));
        order = d_idx_a.get();
    }
    hipLaunchKernelGGL(k_leaves, grid_for(n), dim3(kBlock), 0, nullptr, d_boxes.get(), order, n, d_nodes.get(),
                       d_cluster_a.get(), d_cbox_a.get());
    TRX_BUILD_TRY(hipGetLastError());

    uint32_t *cluster = d_cluster_a.get(), *cluster_next = d_cluster_b.get();
    Aabb *cbox = d_cbox_a.get(), *cbox_next = d_cbox_b.get();
    uint32_t m = n, next_node = n;
    for (uint32_t round = 0; m > 1; round++) {
        const uint32_t r = round < depth_threshold ? 1u : std::max(1u, radius);
        hipLaunchKernelGGL(k_nearest, grid_for(m), dim3(kBlock), 0, nullptr, cbox, m, r, d_nn.get());
        hipLaunchKernelGGL(k_flags, grid_for(m), dim3(kBlock), 0, nullptr, d_nn.get(), m, d_flags.get());
        tb = tmp_bytes;
        TRX_BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.get(), tb, d_flags.get(), d_scan.get(), (int)m, nullptr));
        hipLaunchKernelGGL(k_apply, grid_for(m), dim3(kBlock), 0, nullptr, d_nn.get(), d_flags.get(), d_scan.get(), m,
                           next_node, cluster, cbox, d_nodes.get(), cluster_next, cbox_next);
        TRX_BUILD_TRY(hipGetLastError());
        uint64_t last_scan = 0, last_flag = 0;
        TRX_BUILD_TRY(hipMemcpy(&last_scan, d_scan.get() + (m - 1), 8, hipMemcpyDeviceToHost));
        TRX_BUILD_TRY(hipMemcpy(&last_flag, d_flags.get() + (m - 1), 8, hipMemcpyDeviceToHost));
        const uint64_t sum = last_scan + last_flag;
        const uint32_t m_new = (uint32_t)(sum & 0xffffffffull), merges = (uint32_t)(sum >> 32);
        if (merges == 0 || m_new >= m || (size_t)next_node + merges > total) {
            err = "PLOC round made no progress (device)";
            return false;
        }
        next_node += merges;
        m = m_new;
        std::swap(cluster, cluster_next);
        std::swap(cbox, cbox_next);
    }
    TRX_BUILD_TRY(hipEventRecord(ev1.get(), nullptr));
    uint32_t root = 0;
    TRX_BUILD_TRY(hipMemcpy(&root, cluster, 4, hipMemcpyDeviceToHost));
    TRX_BUILD_TRY(hipMemcpy(nodes_out, d_nodes.get(), total * sizeof(Node2), hipMemcpyDeviceToHost));
    TRX_BUILD_TRY(hipEventSynchronize(ev1.get()));
    float ms = 0.f;
    TRX_BUILD_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
    if (seconds) *seconds = ms * 1e-3;
    if (next_node != total || root != total - 1) {
        err = "PLOC (device) ended with " + std::to_string(next_node) + " nodes, root " + std::to_string(root);
        return false;
    }
    *root_out = root;
    return true;
}

} // namespace trx
