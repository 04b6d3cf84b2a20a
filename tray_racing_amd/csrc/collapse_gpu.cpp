// collapse_gpu.cpp — the last stage of a GPU build: BVH2 -> 8-wide compressed nodes (Ylitie et al. 2017, section 4.2: the
// seven-entry cost table per BVH2 node, then the tree those decisions describe; what obvhs does between its BVH2 and the
// CwBvh the reference uploads, src/main.rs:170-186, and what embree/src/bvh_embree_to_cwbvh.rs:85-186 does for the embree
// builder) as level-synchronous kernels:
//   1. BVH2 levels       top-down frontier expansion; the frontiers are kept, so every level is a list of node ids
//   2. cost table        one thread per node, deepest level first (both children are done when a node runs)
//   3. CWBVH levels      top-down over the collapsed tree: children of a node (distribute decisions followed), octant slot
//                        assignment, one record per node; a node's inner children are consecutive records in slot order
//   4. subtree sizes     bottom-up over the records: nodes and primitives below each record
//   5. output offsets    top-down: the sequential emission (a node's children allocated when it is visited, its primitives
//                        appended then, children visited in slot order) fixes every index as a function of those sizes
//   6. encode            one thread per record: quantisation frame, child boxes, meta bytes, primitive indices
// The decisions, the children of a node, their slots and the encoding are build_rules.h's, the very functions Collapser in
// builder.cpp calls, so the bytes are the host's bytes.
#include "collapse_gpu.h"

#include <algorithm>

#include "build_levels.h"

namespace trx {
namespace {

struct Rec { // one per CWBVH node, in discovery order (level by level)
    uint32_t n2;          // the BVH2 node it is made from
    uint32_t first_child; // record of its first inner child; the others follow in slot order
    uint32_t sub_nodes, sub_prims; // records / primitives in its subtree, itself included
    uint32_t out_idx, child_base, prim_base;
    uint32_t info;        // imask | n_inner << 8 | total_tris << 16
    uint32_t slot_n2[8];  // BVH2 node per slot, kEmpty = none
};
static_assert(sizeof(Rec) == 64, "record size");
constexpr uint32_t kEmpty = 0xffffffffu;

// ---- 2. cost table
__global__ __launch_bounds__(kBlock) void k2_cost(Node2 *nodes, Decision *dec, const uint32_t *list, uint32_t n, uint32_t max_prims,
                                                    float traversal_cost, float prim_cost) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t ni = list[t];
    Node2 nd = load_node(nodes, ni);
    float cl[7], cr[7];
    if (nd.count != 1) { // primitives below: the children (a level down) have theirs; the caller's may be stale
        nd.count = nodes[nd.left].count + nodes[nd.right].count;
        nodes[ni].count = nd.count;
        for (int k = 0; k < 7; k++) {
            cl[k] = dec[(size_t)nd.left * 7 + k].cost;
            cr[k] = dec[(size_t)nd.right * 7 + k].cost;
        }
    }
    collapse_costs(half_area(nd.box), nd.count, cl, cr, max_prims, traversal_cost, prim_cost, dec + (size_t)ni * 7);
}

// ---- 3. CWBVH levels
__global__ __launch_bounds__(kBlock) void k8_expand(const Node2 *nodes, const Decision *dec, Rec *recs, uint32_t begin, uint32_t end,
                                                      uint32_t *n_recs, uint32_t *trouble) {
    const uint32_t r = begin + blockIdx.x * kBlock + threadIdx.x;
    uint32_t n_inner = 0, imask = 0, total_tris = 0;
    uint32_t slot_n2[8];
    for (int s = 0; s < 8; s++) slot_n2[s] = kEmpty;
    if (r < end) {
        const uint32_t ni = recs[r].n2;
        uint32_t children[8];
        const int count = collapsed_children(
            ni, [&](uint32_t i, uint32_t &left, uint32_t &right, uint32_t &cnt) { uint32_t prim; load_links(nodes, i, left, right, prim, cnt); },
            [&](size_t k) { return dec[k]; }, children);
        if (count > 8) {
            atomicOr(trouble, 1u);
        } else {
            int slot_child[8];
            assign_slots(load_node(nodes, ni).box, [&](int c) { return load_node(nodes, children[c]).box; }, count, slot_child);
            for (int s = 0; s < 8; s++) {
                if (slot_child[s] < 0) continue;
                const uint32_t c = children[slot_child[s]];
                slot_n2[s] = c;
                if (dec[(size_t)c * 7].type == kInternal) {
                    imask |= 1u << s;
                    n_inner++;
                } else {
                    uint32_t left, right, prim, cnt;
                    load_links(nodes, c, left, right, prim, cnt);
                    total_tris += cnt;
                }
            }
            if (total_tris > 24) atomicOr(trouble, 2u);
        }
    }
    const uint32_t first = wave_append(n_recs, n_inner);
    if (r < end) {
        Rec &rec = recs[r];
        rec.first_child = first;
        rec.info = imask | (n_inner << 8) | (total_tris << 16);
        uint32_t k = 0;
        for (int s = 0; s < 8; s++) {
            rec.slot_n2[s] = slot_n2[s];
            if (imask & (1u << s)) recs[first + k++].n2 = slot_n2[s];
        }
    }
}

// ---- 4. subtree sizes (deepest level first)
__global__ __launch_bounds__(kBlock) void k8_sizes(Rec *recs, uint32_t begin, uint32_t end) {
    const uint32_t r = begin + blockIdx.x * kBlock + threadIdx.x;
    if (r >= end) return;
    const uint32_t info = recs[r].info, n_inner = (info >> 8) & 0xffu, first = recs[r].first_child;
    uint32_t nodes = 1, prims = info >> 16;
    for (uint32_t k = 0; k < n_inner; k++) {
        nodes += recs[first + k].sub_nodes;
        prims += recs[first + k].sub_prims;
    }
    recs[r].sub_nodes = nodes;
    recs[r].sub_prims = prims;
}

// ---- 5. output offsets (root first).  Collapser::emit visits a node, allocates its inner children at the end of the node
// array, appends its primitives, then visits the children in slot order: child k's own children start after everything
// children 0..k-1 put below themselves.
__global__ __launch_bounds__(kBlock) void k8_offsets(Rec *recs, uint32_t begin, uint32_t end) {
    const uint32_t r = begin + blockIdx.x * kBlock + threadIdx.x;
    if (r >= end) return;
    if (r == 0) {
        recs[0].out_idx = 0;
        recs[0].child_base = 1;
        recs[0].prim_base = 0;
    }
    const uint32_t info = recs[r].info, n_inner = (info >> 8) & 0xffu, first = recs[r].first_child;
    const uint32_t child_base = recs[r].child_base;
    uint32_t next_nodes = child_base + n_inner, next_prims = recs[r].prim_base + (info >> 16);
    for (uint32_t k = 0; k < n_inner; k++) {
        Rec &c = recs[first + k];
        c.out_idx = child_base + k;
        c.child_base = next_nodes;
        c.prim_base = next_prims;
        next_nodes += c.sub_nodes - 1;
        next_prims += c.sub_prims;
    }
}

// ---- 6. encode (Collapser::emit for one node; embree/src/bvh_embree_to_cwbvh.rs:85-186)
__global__ __launch_bounds__(kBlock) void k8_encode(const Node2 *nodes, const Rec *recs, uint32_t n_recs, uint4 *out_nodes, uint32_t *out_prims) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_recs) return;
    const Rec rec = recs[r];
    const Node2 nd = load_node(nodes, rec.n2);
    float e[3], p[3];
    uint32_t ebyte[3];
    for (int k = 0; k < 3; k++) {
        p[k] = frame_origin(nd.box.mn[k]);
        e[k] = quant_step(nd.box.mn[k], nd.box.mx[k]);
        ebyte[k] = (__float_as_uint(e[k]) >> 23) & 0xffu;
    }
    const uint32_t imask = rec.info & 0xffu;
    uint32_t meta[2] = {0, 0}, q[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}; // min_x,max_x,min_y,max_y,min_z,max_z
    uint32_t total_tris = 0;
    for (int s = 0; s < 8; s++) {
        const uint32_t c = rec.slot_n2[s];
        if (c == kEmpty) continue;
        const Node2 ch = load_node(nodes, c);
        for (int k = 0; k < 3; k++) {
            uint32_t lo, hi;
            quant_planes(p[k], e[k], ch.box.mn[k], ch.box.mx[k], lo, hi);
            q[2 * k][s >> 2] |= lo << (8 * (s & 3));
            q[2 * k + 1][s >> 2] |= hi << (8 * (s & 3));
        }
        uint32_t m;
        if (imask & (1u << s)) {
            m = inner_meta(s);
        } else {
            // Collapser::collect_prims: the leaves below c in pre-order (left before right); at most three
            uint32_t st[4];
            int sp = 0;
            st[sp++] = c;
            uint32_t np = 0;
            while (sp > 0) {
                uint32_t left, right, prim, cnt;
                load_links(nodes, st[--sp], left, right, prim, cnt);
                if (cnt == 1) {
                    out_prims[rec.prim_base + total_tris + np] = prim;
                    np++;
                } else {
                    st[sp++] = right;
                    st[sp++] = left;
                }
            }
            m = leaf_meta(total_tris, np);
            total_tris += np;
        }
        meta[s >> 2] |= m << (8 * (s & 3));
    }
    uint4 *o = out_nodes + (size_t)rec.out_idx * 5;
    o[0] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]),
                      ebyte[0] | (ebyte[1] << 8) | (ebyte[2] << 16) | (imask << 24));
    o[1] = make_uint4(rec.child_base, rec.prim_base, meta[0], meta[1]);
    o[2] = make_uint4(q[0][0], q[0][1], q[1][0], q[1][1]);
    o[3] = make_uint4(q[2][0], q[2][1], q[3][0], q[3][1]);
    o[4] = make_uint4(q[4][0], q[4][1], q[5][0], q[5][1]);
}

} // namespace

bool collapse_encode_device(int device, const void *nodes, size_t n_nodes, uint32_t max_prims_per_leaf, float traversal_cost,
                            float prim_cost, std::vector<CwbvhNode> &out_nodes, std::vector<uint32_t> &out_prims,
                            float *root_cost, double *seconds, std::string &err, uint32_t *levels) {
    DeviceScope scope;
    if (!scope.enter(device, err)) return false;
    if (n_nodes < 3 || n_nodes > 0x7fffffffull || (n_nodes & 1) == 0) {
        err = "collapse_encode_device: needs a tree of 2n-1 nodes, n >= 2";
        return false;
    }
    const uint32_t n = (uint32_t)n_nodes, n_prims = (n + 1) / 2;
    DevBuf<Node2> d_nodes;
    DevBuf<Decision> d_dec;
    DevBuf<uint32_t> d_list, d_counter, d_out_prims;
    DevBuf<Rec> d_recs;
    DevBuf<uint4> d_out_nodes;
    Event ev0, ev1;
    TRX_BUILD_TRY(d_nodes.alloc(n));
    TRX_BUILD_TRY(d_dec.alloc((size_t)n * 7));
    TRX_BUILD_TRY(d_list.alloc(n));
    TRX_BUILD_TRY(d_counter.alloc(4));
    // a CWBVH node has at least two children unless it is the root of a one-primitive scene, so there are fewer nodes than
    // primitives
    TRX_BUILD_TRY(d_recs.alloc(n_prims));
    TRX_BUILD_TRY(d_out_prims.alloc(n_prims));
    TRX_BUILD_TRY(ev0.create());
    TRX_BUILD_TRY(ev1.create());
    TRX_BUILD_TRY(hipMemcpy(d_nodes.get(), nodes, (size_t)n * sizeof(Node2), hipMemcpyHostToDevice));
    TRX_BUILD_TRY(hipEventRecord(ev0.get(), nullptr));

    // 1. BVH2 levels: level L = list[level[L] .. level[L + 1])
    std::vector<uint32_t> level;
    if (!expand_levels("collapse_encode_device", d_nodes.get(), n, d_list.get(), d_counter.get(), level, err)) return false;
    // 2. cost table, deepest level first
    for (size_t L = level.size() - 1; L-- > 0;) {
        const uint32_t begin = level[L], end = level[L + 1];
        hipLaunchKernelGGL(k2_cost, grid_for(end - begin), dim3(kBlock), 0, nullptr, d_nodes.get(), d_dec.get(), d_list.get() + begin, end - begin,
                           max_prims_per_leaf, traversal_cost, prim_cost);
    }
    TRX_BUILD_TRY(hipGetLastError());
    // 3. CWBVH levels
    std::vector<uint32_t> level8{0u, 1u};
    {
        const uint32_t first[2] = {1u, 0u}; // records so far; trouble flags
        TRX_BUILD_TRY(hipMemcpy(d_counter.get(), first, 8, hipMemcpyHostToDevice));
        const uint32_t zero = 0;
        TRX_BUILD_TRY(hipMemcpy(&d_recs.get()->n2, &zero, 4, hipMemcpyHostToDevice));
    }
    for (;;) {
        const uint32_t begin = level8[level8.size() - 2], end = level8.back();
        if (end == begin) {
            level8.pop_back();
            break;
        }
        hipLaunchKernelGGL(k8_expand, grid_for(end - begin), dim3(kBlock), 0, nullptr, d_nodes.get(), d_dec.get(), d_recs.get(), begin, end, d_counter.get(), d_counter.get() + 1);
        TRX_BUILD_TRY(hipGetLastError());
        uint32_t state[2] = {0, 0};
        TRX_BUILD_TRY(hipMemcpy(state, d_counter.get(), 8, hipMemcpyDeviceToHost));
        if (state[1] || state[0] > n_prims || state[0] < end) {
            err = "collapse_encode_device: the decisions give a node more than eight children or 24 primitives";
            return false;
        }
        level8.push_back(state[0]);
    }
    const uint32_t n_recs = level8.back();
    if (levels) *levels = (uint32_t)level8.size() - 1u;
    // 4. subtree sizes, 5. output offsets
    for (size_t L = level8.size() - 1; L-- > 0;)
        hipLaunchKernelGGL(k8_sizes, grid_for(level8[L + 1] - level8[L]), dim3(kBlock), 0, nullptr, d_recs.get(), level8[L], level8[L + 1]);
    for (size_t L = 0; L + 1 < level8.size(); L++)
        hipLaunchKernelGGL(k8_offsets, grid_for(level8[L + 1] - level8[L]), dim3(kBlock), 0, nullptr, d_recs.get(), level8[L], level8[L + 1]);
    TRX_BUILD_TRY(hipGetLastError());
    // 6. encode
    static_assert(sizeof(CwbvhNode) == 5 * sizeof(uint4), "a node is five uint4");
    TRX_BUILD_TRY(d_out_nodes.alloc((size_t)n_recs * 5));
    hipLaunchKernelGGL(k8_encode, grid_for(n_recs), dim3(kBlock), 0, nullptr, d_nodes.get(), d_recs.get(), n_recs, d_out_nodes.get(), d_out_prims.get());
    TRX_BUILD_TRY(hipGetLastError());
    TRX_BUILD_TRY(hipEventRecord(ev1.get(), nullptr));
    Rec root;
    TRX_BUILD_TRY(hipMemcpy(&root, d_recs.get(), sizeof(Rec), hipMemcpyDeviceToHost));
    if (root.sub_nodes != n_recs || root.sub_prims != n_prims) {
        err = "collapse_encode_device: subtree sizes do not add up";
        return false;
    }
    out_nodes.resize(n_recs);
    out_prims.resize(n_prims);
    TRX_BUILD_TRY(hipMemcpy(out_nodes.data(), d_out_nodes.get(), (size_t)n_recs * sizeof(CwbvhNode), hipMemcpyDeviceToHost));
    TRX_BUILD_TRY(hipMemcpy(out_prims.data(), d_out_prims.get(), (size_t)n_prims * 4, hipMemcpyDeviceToHost));
    if (root_cost) {
        Decision d0;
        TRX_BUILD_TRY(hipMemcpy(&d0, d_dec.get(), sizeof(Decision), hipMemcpyDeviceToHost));
        *root_cost = d0.cost;
    }
    if (seconds) {
        float ms = 0.f;
        TRX_BUILD_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        *seconds += ms * 1e-3;
    }
    return true;
}

} // namespace trx
